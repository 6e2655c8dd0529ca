"""Directed pairs with a circle: one manifold each, named for the arm of the round narrowphase it reaches (narrowphase.h
circle_circle_contact / circle_box_contact, merge_point and the two-slot store; tests/circle_spec.py states them).
tests/test_circles_cpu.py holds phx_debug_update_manifold — the host instantiation of the function the device kernel calls — to the
spec byte for byte on every case, checks that each case reaches the arm it is named for, and holds the spec to the float64 judge
(tests/circle_reference.py).

A case is a Case below: two 128-byte records with their kinds, the manifold's cached point count and its two contact-point slots, and
the claim `expect` = (point count after the update, is_newly_created of slot 0) with `arm`, the branch the new point comes from:
  cc          circle/circle, l > 0                      cc_miss     l2 > R*R
  cc_centre   concentric circles (l == 0, n = (1, 0))
  face        circle/box, the centre beyond one face    corner      beyond two faces
  miss        circle/box, l2 > r*r
  in_x, in_y  the centre inside the box, the face on x (pu <= pv) / on y;  in_tie: pu == pv (x wins);  on_face: u == h.x exactly
Every circle/box case exists with the circle as body 1 and as body 2 (`_b2`), and with the box's frame as it is, a quarter turn on
(`_q`, exact: xv = (0, 1), yv = (-1, 0)) and turned by an inexact angle (`_t`, xv = (0.8, 0.6)f); the exact ties and the centre on a
face exist only with the exact frames, where the rounded u and v are the intended ones.  Cache cases (`cache_*`) start from a cached
point: matched (merged, not new, solver_index and padding kept), farther than the merge distance (a new point in slot 0), two
cached points of a box/box past of which the nearer one survives, and two far ones (the new point is the third of the working set).

Measured: the spec's worst deviation from the float64 judge over the cases of each group, in the measures of
circle_reference.deviation (`length`: | |n| - 1 |, `normal`: radians, `depth` and `surface`: relative to the pair's scale).  The
test's bound is the figure below times 4, the allowance for other libm and numpy builds (sqrt and / are correctly rounded
everywhere; what may differ is the float64 side).  A figure of 0 is bounded by 4 * 2^-24 = 2.4e-07, four float32 half-ulps.
The C++ is the spec byte for byte, so its deviations are these.
  group            cases     length     normal      depth    surface
  circle/circle        6   2.38e-08   1.53e-08   6.79e-08   4.45e-08
  circle/box          70   2.38e-08   6.67e-08   4.29e-08   4.24e-08
  cache                5          0          0          0          0
"""
import numpy as np

from phyx_amd.api import contact_point_dtype, rigid_body_dtype

F = np.float32
BOX, CIRCLE = 0, 1
FACTOR = 4.0
FLOOR = 2.0 ** -24
# group -> (length, normal, depth, surface): the table above, as numbers
MEASURED = {
    "circle/circle": (2.38e-08, 1.53e-08, 6.79e-08, 4.45e-08),
    "circle/box": (2.38e-08, 6.67e-08, 4.29e-08, 4.24e-08),
    "cache": (0.0, 0.0, 0.0, 0.0),
}

FRAMES = {"": ((1.0, 0.0), (0.0, 1.0)), "_q": ((0.0, 1.0), (-1.0, 0.0)), "_t": ((0.8, 0.6), (-0.6, 0.8))}


def record(pos, size, frame=FRAMES[""]):
    b = np.zeros(1, dtype=rigid_body_dtype)[0]
    b["pos"]["x"], b["pos"]["y"] = pos
    b["xv"]["x"], b["xv"]["y"] = frame[0]
    b["yv"]["x"], b["yv"]["y"] = frame[1]
    b["geom_size"]["x"], b["geom_size"]["y"] = size
    b["geom_pos"], b["geom_xv"], b["geom_yv"] = b["pos"], b["xv"], b["yv"]
    return b


def blank_points():
    p = np.zeros(2, dtype=contact_point_dtype)
    p["solver_index"] = -1
    return p


class Case:
    def __init__(self, name, group, arm, b1, k1, b2, k2, expect, count=0, pts=None):
        self.name, self.group, self.arm = name, group, arm
        self.b1, self.k1, self.b2, self.k2 = b1, k1, b2, k2
        self.count, self.pts = count, blank_points() if pts is None else pts
        self.expect = expect


def _world(local, frame, origin):
    """The float32 world point of the box-frame point `local` (float64 arithmetic, rounded once)."""
    x = origin[0] + frame[0][0] * local[0] + frame[1][0] * local[1]
    y = origin[1] + frame[0][1] * local[0] + frame[1][1] * local[1]
    return (float(F(x)), float(F(y)))


def _circle_box(name, arm, local, expect, frames, r=4.0, h=(5.0, 3.0), origin=(20.0, -10.0)):
    out = []
    for tag in frames:
        fr = FRAMES[tag]
        box = record(origin, h, fr)
        circle = record(_world(local, fr, origin), (r, r), FRAMES["_t"])      # (a circle's own frame is never read)
        out.append(Case(name + tag, "circle/box", arm, circle, CIRCLE, box, BOX, expect))
        out.append(Case(name + tag + "_b2", "circle/box", arm, box, BOX, circle, CIRCLE, expect))
    return out


def _cached(d1, d2, n, si, pad=(0, 0), merged=1, new=0):
    p = np.zeros(1, dtype=contact_point_dtype)[0]
    p["delta1"]["x"], p["delta1"]["y"] = d1
    p["delta2"]["x"], p["delta2"]["y"] = d2
    p["normal"]["x"], p["normal"]["y"] = n
    p["is_merged"], p["is_newly_created"], p["pad"], p["solver_index"] = merged, new, pad, si
    return p


def cases():
    cs = []
    hit, none = (1, 1), (0, None)
    # ---- circle/circle: r1 = 4, r2 = 6, R = 10, R*R = 100 ----
    up, down = float(np.nextafter(F(10), F(np.inf))), float(np.nextafter(F(10), F(0)))
    for name, arm, p1, expect in (("cc_below", "cc", (down, 0.0), hit), ("cc_at", "cc", (10.0, 0.0), hit), ("cc_above", "cc_miss", (up, 0.0), none),
                                  ("cc_at_diagonal", "cc", (6.0, 8.0), hit), ("cc_deep", "cc", (-3.0, 2.5), hit), ("cc_far", "cc_miss", (30.0, 1.0), none)):
        cs.append(Case(name, "circle/circle", arm, record(p1, (4.0, 4.0)), CIRCLE, record((0.0, 0.0), (6.0, 6.0)), CIRCLE, expect))
    cs.append(Case("cc_offset", "circle/circle", "cc", record((1003.5, -2001.25), (4.0, 4.0)), CIRCLE, record((1000.0, -1995.0), (6.0, 6.0)), CIRCLE, hit))
    cs.append(Case("cc_concentric", "circle/circle", "cc_centre", record((7.0, 7.0), (4.0, 4.0)), CIRCLE, record((7.0, 7.0), (6.0, 6.0)), CIRCLE, hit))
    # ---- circle/box: r = 4, h = (5, 3) ----
    every, exact = ("", "_q", "_t"), ("", "_q")
    cs += _circle_box("face_x", "face", (8.5, 1.0), hit, every)
    cs += _circle_box("face_x_neg", "face", (-8.5, -1.0), hit, every)
    cs += _circle_box("face_y", "face", (-2.0, 6.0), hit, every)
    cs += _circle_box("corner", "corner", (7.5, 5.5), hit, every)
    cs += _circle_box("corner_neg", "corner", (-7.5, -5.5), hit, every)
    cs += _circle_box("corner_miss", "miss", (8.5, 6.5), none, every)
    cs += _circle_box("face_miss", "miss", (9.5, 0.0), none, every)
    cs += _circle_box("inside_x", "in_x", (4.0, 0.5), hit, every)
    cs += _circle_box("inside_x_neg", "in_x", (-4.0, 0.5), hit, every)
    cs += _circle_box("inside_y", "in_y", (0.5, 2.5), hit, every)
    cs += _circle_box("inside_y_neg", "in_y", (0.5, -2.5), hit, every)
    cs += _circle_box("inside_tie", "in_tie", (3.0, 1.0), hit, exact)
    cs += _circle_box("inside_centre", "in_y", (0.0, 0.0), hit, exact)
    cs += _circle_box("on_face", "on_face", (5.0, 1.0), hit, exact)
    cs += _circle_box("on_corner", "on_face", (5.0, 3.0), hit, exact)
    # ---- the cache: circle (body 1, r = 4) at (8.5, 1) of an axis-aligned box h = (5, 3) at the origin: the new point has
    #      delta1 = (-4, 0), delta2 = (5, 1), n = (1, 0) ----
    circle, box = record((8.5, 1.0), (4.0, 4.0)), record((0.0, 0.0), (5.0, 3.0))
    near = _cached((-3.5, 0.5), (5.0, 1.5), (0.0, 1.0), 7, pad=(3, 9))
    far = _cached((-3.0, 4.0), (5.0, -3.0), (1.0, 0.0), 11)
    far2 = _cached((0.0, -4.0), (-5.0, 3.0), (1.0, 0.0), 12, new=1)

    def pts(*p):
        a = blank_points()
        for k, q in enumerate(p):
            a[k] = q
        return a
    cs.append(Case("cache_matched", "cache", "face", circle, CIRCLE, box, BOX, (1, 0), 1, pts(near)))
    cs.append(Case("cache_far", "cache", "face", circle, CIRCLE, box, BOX, (1, 1), 1, pts(far)))
    cs.append(Case("cache_box_past", "cache", "face", circle, CIRCLE, box, BOX, (1, 0), 2, pts(far, near)))
    cs.append(Case("cache_two_far", "cache", "face", circle, CIRCLE, box, BOX, (1, 1), 2, pts(far, far2)))
    cs.append(Case("cache_dropped", "cache", "miss", record((9.5, 0.0), (4.0, 4.0)), CIRCLE, box, BOX, (0, None), 2, pts(near, far)))
    cs.append(Case("cache_cc_matched", "cache", "cc", record((9.0, 0.0), (4.0, 4.0)), CIRCLE, record((0.0, 0.0), (6.0, 6.0)), CIRCLE, (1, 0), 1,
                   pts(_cached((-4.0, 1.0), (6.0, 1.0), (1.0, 0.0), 3))))
    return cs
