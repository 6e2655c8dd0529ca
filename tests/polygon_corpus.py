"""Directed pairs with a convex polygon: one manifold each, named for the arm of the polygon narrowphase it reaches (narrowphase.h
polygon_polygon_contact / disc_polygon_cand / capsule_polygon_cand / select_stream, merge_point and the two-slot store;
tests/polygon_spec.py states them).  tests/test_polygons_cpu.py holds phx_debug_update_manifold_polygons to the spec byte for byte on
every case, checks that each case reaches the arm it is named for, and holds the spec to the float64 judge (tests/polygon_reference.py).

A case is a Case below: two 128-byte records with their kinds and polygons, the manifold's cached point count and its two contact-point
slots, and the claim: `expect` = (point count after the update, is_newly_created of the stored slots) and `arm`, a dict of what the
spec's trace must show (polygon_spec.poly_poly / disc_polygon / capsule_polygon with capsule_spec.select):
  polygon/polygon   ref ("A", "B", None: apart), kept (points that pass s <= 0), clips (the ends the two side planes cut: the
                    incident edge faces the reference edge and runs against it, so the first plane, at the reference edge's start,
                    can only cut the incident edge's end, lo:p1, and the second its start, hi:p0),
                    ab_tie (sB == sA), face_tie, inc_tie, touch (s == 0)
  circle/polygon    region (inside, face, vertex_lo, vertex_hi, None: no candidate), tie, t0 / tee (t == 0, t == dot(e, e)),
                    touch (l2 == r*r)
  capsule/polygon   first / second (end0, end1, vertex<k>; None), clamped (vertices met nearest an end of the core: not counted),
                    depth_tie / sep_tie, rejected
Every scene exists in both body orders (`_b2`: ref A <-> B) and under the whole-scene frames of circle_corpus.FRAMES: as it is, a
quarter turn on (`_q`, exact) and turned by an inexact angle (`_t`); scenes that rest on an exact tie or an exact boundary exist under
the exact frames only (the one-ulp gap under the plain frame alone: a turned coordinate rounds it away).

One property of the rule shows in pp_face_tie: the two kept points lie 0.5 apart, the second goes through MergeCollision like the
first and merges into it (the two are Equals under 2.0f), and a point that was merged into is no longer marked newly created: the pair
stores one point, with the second's position and is_newly_created 0 in the step that made it.  Only the contact reports' NEW flag reads
that mark; the joint is matched by its solver index, which stays -1.

Measured: the spec's worst deviation from the float64 judge over the cases of each group, in the four measures of
polygon_reference.deviation (`depth` for each pair's deepest point; a capsule pair's second point keeps its own candidate's normal, as in
capsule_corpus, and is held to `length` and `surface`).  The test's bound is the figure times FACTOR = 4, a figure under
FLOOR = 2^-24 counting as the floor (circle_corpus has the reasons).  The C++ is the spec byte for byte, so its deviations are these.
Figures that are not rounding, and are the rule's own:
  - capsule/polygon `surface` 1.25e-4 (times the scale, 20: 2.5e-3): a second point that comes from an end disc lies on that disc's
    circle along the contact normal, r * (1 - cos(theta)) inside the capsule's side where the normal leans by theta from the side's own
    (theta = 0.05, r = 2): the capsule rule's own term (capsule_corpus), of second order in the lean and zero at rest.
  - capsule/polygon `normal` 9.2e-07 rad (kp_end_at_vertex_t: an end disc 1.41 from the tray's corner): an end's centre is formed in
    fp32 and the normal is that rounding seen from the distance l (capsule_corpus has the same figure for a box's corner).
  group              cases     length     normal      depth    surface
  polygon/polygon       90   2.71e-08   1.11e-16   8.02e-08   7.62e-08
  circle/polygon        72   4.53e-08   4.77e-08   3.76e-08    5.1e-08
  capsule/polygon       60   5.03e-08   9.16e-07   5.13e-08   0.000125
  cache                  3          0          0          0          0
(polygon/polygon `normal` is exact here: a world normal is xv*n.x + yv*n.y of a frame whose yv is perp(xv) bit for bit, which is the
direction the judge gets from the same frame's edges; the figure counts as the floor.)
"""
import numpy as np

import circle_corpus as cc
import polygon_spec as spec
from capsule_corpus import EVERY, EXACT, FLAT, UP, _cached, _pts, body, place
from circle_corpus import blank_points, record

F = np.float32
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
FACTOR = cc.FACTOR
FLOOR = cc.FLOOR
# group -> (length, normal, depth, surface)
MEASURED = {
    "polygon/polygon": (2.71e-08, 1.11e-16, 8.02e-08, 7.62e-08),
    "circle/polygon": (4.53e-08, 4.77e-08, 3.76e-08, 5.1e-08),
    "capsule/polygon": (5.03e-08, 9.16e-07, 5.13e-08, 1.25e-04),
    "cache": (0.0, 0.0, 0.0, 0.0),
}
PLAIN = ("",)

GROUND = spec.polygon([(-12, -3), (12, -3), (10, 3), (-10, 3)])             # a trapezoid tray, top face y = 3 from x = -10 to 10
SQUARE = spec.polygon([(-4, -4), (4, -4), (4, 4), (-4, 4)])
SQUARE3 = spec.polygon([(-3, -3), (3, -3), (3, 3), (-3, 3)])
DIAMOND = spec.polygon([(0, -5), (4, 0), (0, 5), (-4, 0)])
TRIANGLE = spec.polygon([(-6, -3), (6, -3), (0, 6)])
OCTAGON = spec.regular(8, 5.0, np.pi / 8)                                   # flat on top and below: the faces at y = -+5 cos(pi/8)


class Case:
    def __init__(self, name, group, b1, k1, p1, b2, k2, p2, expect, arm, count=0, pts=None):
        self.name, self.group = name, group
        self.b1, self.k1, self.p1, self.b2, self.k2, self.p2 = b1, k1, p1, b2, k2, p2
        self.count, self.pts = count, blank_points() if pts is None else pts
        self.expect, self.arm = expect, dict(arm)


def poly(p, pos, angle=FLAT):
    hx, hy = spec.frame_box(p)
    b = body(POLYGON, pos, (float(hx), float(hy)), angle)
    b["poly"] = p
    return b


def _swapped(arm):
    """The claim as the exchanged body order sees it: the reference body changes its name; a tie between sA and sB changes the
    reference body itself (A wins it), which `ref_on_tie` allows for."""
    out = dict(arm)
    if arm.get("ref") in ("A", "B") and not arm.get("ab_tie"):
        out["ref"] = "B" if arm["ref"] == "A" else "A"
    return out


def scene(name, group, one, two, count, arm, frames, swapped=None, new=None):
    """The scene in both body orders under `frames`; `swapped`: the claim with the bodies exchanged, where it is not _swapped(arm);
    `new`: the stored slots' is_newly_created, where not every stored point is new."""
    out = []
    for tag in frames:
        r1, r2 = place(one, tag), place(two, tag)
        for suffix, a, ra, b, rb, claim in (("", one, r1, two, r2, arm), ("_b2", two, r2, one, r1, swapped if swapped is not None else _swapped(arm))):
            out.append(Case(name + tag + suffix, group, ra, a["kind"], a.get("poly"), rb, b["kind"], b.get("poly"), (count, (1,) * count if new is None else new), claim))
    return out


def cases():
    cs = []
    ground = poly(GROUND, (0.0, 0.0))
    # ---- polygon/polygon ----
    g = "polygon/polygon"
    cs += scene("pp_face_on_face", g, poly(SQUARE, (0.0, 6.5)), ground, 2, {"ref": "A", "kept": 2, "ab_tie": True, "clips": ["lo:p1", "hi:p0"]}, EXACT,
                swapped={"ref": "A", "kept": 2, "ab_tie": True, "clips": []})
    cs += scene("pp_lean", g, poly(SQUARE, (0.0, 6.6), 0.05), ground, 2, {"ref": "B", "kept": 2}, EVERY)
    cs += scene("pp_lean_back", g, poly(SQUARE, (0.0, 6.6), -0.05), ground, 2, {"ref": "B", "kept": 2}, EVERY)
    cs += scene("pp_vertex_on_face", g, poly(DIAMOND, (0.0, 7.5)), ground, 1, {"ref": "B", "kept": 1, "inc_tie": True}, EXACT)
    cs += scene("pp_vertex_on_face_turned", g, poly(DIAMOND, (0.0, 7.5), 0.1), ground, 1, {"ref": "B", "kept": 1}, EVERY)
    # (the tray's top is the reference and runs from (10, 3) to (-10, 3): its first side plane, at x = 10, cuts the square's far corner)
    cs += scene("pp_partial_right", g, poly(SQUARE, (10.0, 6.6), 0.05), ground, 2, {"ref": "B", "kept": 2, "clips": ["lo:p1"]}, EVERY)
    # (the square's lowest corner hangs beyond the tray's end: its own bottom face is the shallower one and the reference; its second
    #  side plane, at its inner corner, cuts the tray's top)
    cs += scene("pp_partial_left", g, poly(SQUARE, (-10.0, 6.6), 0.05), ground, 2, {"ref": "A", "kept": 2, "clips": ["hi:p0"]}, EVERY)
    cs += scene("pp_partial_left_back", g, poly(SQUARE, (-10.0, 6.6), -0.05), ground, 2, {"ref": "B", "kept": 2, "clips": ["hi:p0"]}, EVERY)
    cs += scene("pp_partial_tie_right", g, poly(SQUARE, (10.0, 6.5)), ground, 2, {"ref": "A", "kept": 2, "ab_tie": True, "clips": ["lo:p1"]}, EXACT)
    cs += scene("pp_partial_tie_left", g, poly(SQUARE, (-10.0, 6.5)), ground, 2, {"ref": "A", "kept": 2, "ab_tie": True, "clips": ["hi:p0"]}, EXACT)
    cs += scene("pp_tri_oct", g, poly(TRIANGLE, (0.0, 0.0)), poly(OCTAGON, (0.0, -7.5)), 2, {"kept": 2}, EVERY)
    cs += scene("pp_box_on_polygon", g, body(BOX, (0.0, 5.5), (5.0, 3.0)), ground, 2, {"ref": "A", "kept": 2, "ab_tie": True}, EXACT)
    cs += scene("pp_box_on_polygon_lean", g, body(BOX, (0.0, 5.6), (5.0, 3.0), 0.05), ground, 2, {"ref": "B", "kept": 2}, EVERY)
    cs += scene("pp_polygon_on_box", g, poly(OCTAGON, (0.0, 7.5)), body(BOX, (0.0, 0.0), (10.0, 3.0)), 2, {"kept": 2}, EVERY)
    cs += scene("pp_gap_one_ulp", g, poly(SQUARE, (0.0, float(np.nextafter(F(7.0), F(8.0))))), ground, 0, {"ref": None}, PLAIN)
    cs += scene("pp_touching", g, poly(SQUARE, (0.0, 7.0)), ground, 2, {"ref": "A", "kept": 2, "ab_tie": True, "touch": True}, EXACT)
    cs += scene("pp_face_tie", g, poly(SQUARE, (7.5, 7.5)), poly(SQUARE, (0.0, 0.0)), 1, {"ref": "A", "kept": 2, "ab_tie": True, "face_tie": True}, EXACT, new=(0,))
    cs += scene("pp_apart", g, poly(SQUARE, (0.0, 9.0)), ground, 0, {"ref": None}, EVERY)
    # ---- circle/polygon: the square {4, 4}, r = 3 unless said ----
    g = "circle/polygon"
    sq = poly(SQUARE, (0.0, 0.0))
    disc = lambda pos, r=3.0: body(CIRCLE, pos, (r, r), 0.6435)      # noqa: E731  (a circle's own frame is never read)
    for name, pos, r, count, arm, frames in (
            ("cp_face", (1.0, 6.5), 3.0, 1, {"region": "face"}, EVERY),
            ("cp_vertex_hi", (6.0, 5.5), 3.0, 1, {"region": "vertex_hi"}, EVERY),
            ("cp_vertex_lo", (-5.5, -6.0), 3.0, 1, {"region": "vertex_lo"}, EVERY),
            ("cp_vertex_hi_tie", (6.0, 6.0), 3.0, 1, {"region": "vertex_hi", "tie": True}, EXACT),
            ("cp_vertex_lo_tie", (-6.0, -6.0), 3.0, 1, {"region": "vertex_lo", "tie": True}, EXACT),
            ("cp_t0", (6.0, -4.0), 3.0, 1, {"region": "face", "t0": True}, EXACT),
            ("cp_tee", (6.0, 4.0), 3.0, 1, {"region": "face", "tee": True}, EXACT),
            ("cp_inside", (1.0, 2.0), 3.0, 1, {"region": "inside"}, EVERY),
            ("cp_touch_vertex", (7.0, 8.0), 5.0, 1, {"region": "vertex_lo", "touch": True}, EXACT),
            ("cp_touch_face", (0.0, 7.0), 3.0, 1, {"region": "face"}, EXACT),
            ("cp_vertex_miss", (6.5, 6.5), 3.0, 0, {"region": None}, EVERY),
            ("cp_miss", (0.0, 8.0), 3.0, 0, {"region": None}, EVERY)):
        cs += scene(name, g, disc(pos, r), sq, count, arm, frames)
    cs += scene("cp_octagon", g, disc((4.5, 4.5)), poly(OCTAGON, (0.0, 0.0)), 1, {"region": "face"}, EVERY)
    cs += scene("cp_triangle_tip", g, disc((0.0, 8.0)), poly(TRIANGLE, (0.0, 0.0)), 1, {}, EVERY)
    # ---- capsule/polygon: K = {8, 2} (a = 6, r = 2) ----
    g = "capsule/polygon"
    K = lambda pos, angle=FLAT, size=(8.0, 2.0): body(CAPSULE, pos, size, angle)      # noqa: E731
    cs += scene("kp_flat", g, K((0.0, 4.5)), ground, 2, {"first": "end0", "second": "end1", "depth_tie": True}, EXACT)
    cs += scene("kp_lean", g, K((0.0, 4.5), 0.05), ground, 2, {"first": "end0", "second": "end1"}, EVERY)
    cs += scene("kp_lean_back", g, K((0.0, 4.5), -0.05), ground, 2, {"first": "end1", "second": "end0"}, EVERY)
    cs += scene("kp_end_at_vertex", g, K((17.0, 4.0)), ground, 1, {"first": "end0", "second": None}, EVERY)
    cs += scene("kp_vertex_into_side", g, K((0.0, 0.0)), poly(DIAMOND, (1.0, 6.5)), 1, {"first": "vertex0", "second": None, "clamped": []}, EVERY)
    cs += scene("kp_vertex_at_end", g, K((0.0, 0.0)), poly(DIAMOND, (7.5, 6.0)), 1, {"first": "end1", "second": None, "clamped": ["vertex0"]}, EVERY)
    cs += scene("kp_sep_tie", g, K((0.0, 8.0), UP, (9.0, 3.0)), poly(SQUARE3, (0.0, 0.0)), 2, {"first": "end0", "second": "vertex2", "sep_tie": True}, EXACT)
    cs += scene("kp_short", g, K((0.0, 4.5), FLAT, (3.0, 2.0)), ground, 1, {"first": "end0", "second": None, "depth_tie": True, "rejected": [("end1", False, False)]}, EXACT)
    cs += scene("kp_across", g, K((0.5, 6.5), 0.05), poly(SQUARE3, (0.0, 2.0)), 2, {"first": "vertex3", "second": "vertex2"}, EVERY)
    cs += scene("kp_across_back", g, K((0.5, 6.5), -0.05), poly(SQUARE3, (0.0, 2.0)), 2, {"first": "vertex2", "second": "vertex3"}, EVERY)
    cs += scene("kp_miss", g, K((0.0, 5.5)), ground, 0, {"first": None, "second": None}, EVERY)
    # ---- the cache: the square (body 1) face on face on the tray at the scene's origin, as pp_face_on_face without the offset: the tie
    #      makes the square's bottom face the reference; the incident edge is the tray's top from (10, 3) to (-10, 3), cut to x = 4 and
    #      x = -4: the new points are {delta1 (4, -4), delta2 (4, 3)} and {delta1 (-4, -4), delta2 (-4, 3)}, n = (0, 1) ----
    top, tray = record((0.0, 6.5), (4.0, 4.0)), record((0.0, 0.0), (12.0, 3.0))
    near0 = _cached((4.5, -4.0), (4.5, 3.0), (1.0, 0.0), 7, pad=(3, 9))
    near1 = _cached((-3.5, -4.0), (-3.5, 3.0), (1.0, 0.0), 8, pad=(1, 2))
    far = _cached((0.0, -4.0), (0.0, 3.0), (0.0, 1.0), 11)

    def cache(name, expect, count, pts, b1=top):
        cs.append(Case(name, "cache", b1, POLYGON, SQUARE, tray, POLYGON, GROUND, expect, {}, count, pts))
    cache("cache_matched", (2, (0, 0)), 2, _pts(near0, near1))
    cache("cache_far", (2, (1, 1)), 1, _pts(far))
    cache("cache_dropped", (0, ()), 2, _pts(near0, far), record((0.0, 12.0), (4.0, 4.0)))
    return cs
