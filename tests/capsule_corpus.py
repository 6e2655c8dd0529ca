"""Directed pairs with a capsule: one manifold each, named for the arm of the capsule narrowphase it reaches (narrowphase.h
disc_box_cand / disc_capsule_cand / capsule_select, merge_point and the two-slot store; tests/capsule_spec.py states them).
tests/test_capsules_cpu.py holds phx_debug_update_manifold to the spec byte for byte on every case, checks that each case reaches the
arm it is named for, and holds the spec to the float64 judge (tests/capsule_reference.py).

A case is a Case below: two 128-byte records with their kinds, the manifold's cached point count and its two contact-point slots, and
the claim: `expect` = (point count after the update, is_newly_created of the stored slots), `first` / `second` = the names of the
candidates selected (capsule_spec.candidates: end0, end1, other0, other1, corner0 .. corner3, circle; None: no such point), and
`flags`, what else the case is there for:
  depth_tie / sep_tie     two candidates of equal depth / two second candidates equally far: the first in order wins
  rejected:<name>:<s1><s2>   candidate <name> is not distinct from the first: s1, s2 = f (that half of the > 4.0f test fails) or t
  clamped:<name>          the candidate's disc meets the capsule, but nearest an end of the core: it does not count
  at_end                  a circle meets the capsule nearest an end of the core (clamped): it counts all the same
  at_a                    a disc's u is exactly +a or -a: unclamped, it counts
  on_core                 l == 0: the disc's centre lies on the core, N = yv
  inside                  an end's centre lies inside the box: the centre-inside branch
  touch                   l2 == R*R exactly: a point of depth 0
  near_circle             a = one ulp of hy
  crossed                 the cores themselves cross (the known limit: the judge claims only that the points lie on the surfaces)
Every scene exists in both body orders (`_b2`) and under the whole-scene frames of circle_corpus.FRAMES: as it is, a quarter turn on
(`_q`, exact) and turned by an inexact angle (`_t`); scenes that rest on an exact tie or an exact boundary exist under the exact frames
only.  Cache cases (`cache2_*`) start from cached points, with two new points this time.

Measured: the spec's worst deviation from the float64 judge over the cases of each group, first points in the four measures of
capsule_reference.deviation, second points in the four of capsule_reference.second (`across`: the component of p2 - p1 across n over
the scale; `disc`: the distance from the surface or from an end disc's circle).  The test's bound is the figure times FACTOR = 4, a
figure under FLOOR = 2^-24 counting as the floor (circle_corpus has the reasons).  The C++ is the spec byte for byte, so its
deviations are these.  Two figures are not rounding at the scale of the others, and both are the rule's own:
  - `normal` of a first point reaches 9.2e-07 rad (kb_corner_clamped_t: an end disc 1.41 from a box's corner, coordinates near 30).
    An end's centre is formed in fp32 (pos -+ xv*a, 2^-24 * 30 = 1.8e-6 of rounding), the judge's is exact, and the normal is that
    offset seen from 1.41 away.  A circle's centre is a stored value and has no such term.
  - `surface` of a second point is 1.25e-4 and 1.87e-4 (times the scale, 20: 2.5e-3 and 3.7e-3) in the leaning scenes: a second point
    from an end disc lies on that disc's circle along the contact normal, r * (1 - cos(theta)) inside the capsule's side where the
    normal leans by theta from the side's own (theta = 0.05 here, r = 2 and 3).  `disc` measures the same points against the circle
    they are on and stays at rounding.  The rule is kept: the term is of second order in the lean and zero at rest.
  group            cases     length     normal      depth    surface  |  seconds     length    surface       disc     across
  capsule/box         96   5.03e-08   9.16e-07   7.16e-08   7.14e-08  |       66   2.71e-08   0.000125   6.55e-08   5.47e-08
  capsule/circle      44   6.72e-08   8.42e-08   5.78e-08   5.66e-08  |        0          0          0          0          0
  capsule/capsule     48   2.38e-08   3.62e-07   3.79e-08   3.93e-08  |       28   2.71e-08   0.000187    4.3e-08   9.42e-09
  cache                4          0          0          0          0  |        4          0          0          0          0
"""
import numpy as np

import circle_corpus as cc
from circle_corpus import FRAMES, blank_points, record

F = np.float32
BOX, CIRCLE, CAPSULE = 0, 1, 2
FACTOR = cc.FACTOR
FLOOR = cc.FLOOR
# group -> ((length, normal, depth, surface) of the first points, (length, surface, disc, across) of the second points)
MEASURED = {
    "capsule/box": ((5.03e-08, 9.16e-07, 7.16e-08, 7.14e-08), (2.71e-08, 1.25e-04, 6.55e-08, 5.47e-08)),
    "capsule/circle": ((6.72e-08, 8.42e-08, 5.78e-08, 5.66e-08), (0.0, 0.0, 0.0, 0.0)),
    "capsule/capsule": ((2.38e-08, 3.62e-07, 3.79e-08, 3.93e-08), (2.71e-08, 1.87e-04, 4.3e-08, 9.42e-09)),
    "cache": ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)),
}
ORIGIN = (20.0, -10.0)
EVERY, EXACT = ("", "_q", "_t"), ("", "_q")
FLAT, UP, DOWN = 0.0, "up", "down"      # a body's own frame: an angle in radians, or the exact quarter turns xv = (0, 1) / (0, -1)


class Case:
    def __init__(self, name, group, b1, k1, b2, k2, expect, first, second, flags=(), count=0, pts=None):
        self.name, self.group = name, group
        self.b1, self.k1, self.b2, self.k2 = b1, k1, b2, k2
        self.count, self.pts = count, blank_points() if pts is None else pts
        self.expect, self.first, self.second, self.flags = expect, first, second, tuple(flags)
        self.arm = "%s>%s" % (first, second)


def _own_frame(angle):
    if angle == UP:
        return (0.0, 1.0), (-1.0, 0.0)
    if angle == DOWN:
        return (0.0, -1.0), (1.0, 0.0)
    c, s = (1.0, 0.0) if angle == 0.0 else (float(np.cos(angle)), float(np.sin(angle)))
    return (c, s), (-s, c)


def body(kind, pos, size, angle=FLAT):
    return {"kind": kind, "pos": pos, "size": size, "frame": _own_frame(angle)}


def place(b, tag):
    """The record of scene body b under the whole-scene frame `tag` (float64 arithmetic, rounded once)."""
    gx, gy = FRAMES[tag]
    turn = lambda v: (float(F(gx[0] * v[0] + gy[0] * v[1])), float(F(gx[1] * v[0] + gy[1] * v[1])))      # noqa: E731
    pos = (float(F(ORIGIN[0] + gx[0] * b["pos"][0] + gy[0] * b["pos"][1])), float(F(ORIGIN[1] + gx[1] * b["pos"][0] + gy[1] * b["pos"][1])))
    return record(pos, b["size"], (turn(b["frame"][0]), turn(b["frame"][1])))


def scene(name, group, one, two, claim, frames, swapped=None, flags=(), swapped_flags=None):
    """The scene in both body orders under `frames`.  claim = (count, first, second); `swapped`: the claim with the bodies exchanged
    (candidate names depend on the order only where both are capsules)."""
    out = []
    for tag in frames:
        r1, r2 = place(one, tag), place(two, tag)
        for suffix, (ra, ka, rb, kb), (n, first, second) in (("", (r1, one["kind"], r2, two["kind"]), claim),
                                                             ("_b2", (r2, two["kind"], r1, one["kind"]), swapped or claim)):
            fl = (swapped_flags if swapped_flags is not None else tuple(_swap_halves(f) for f in flags)) if suffix else flags
            out.append(Case(name + tag + suffix, group, ra, ka, rb, kb, (n, (1,) * n), first, second, fl))
    return out


def _swap_halves(flag):
    """rejected:<name>:<s1><s2> as the exchanged order sees it: the halves change places (and end <-> other stays with the caller)."""
    if not flag.startswith("rejected:"):
        return flag
    _, name, halves = flag.split(":")
    return "rejected:%s:%s" % (name, halves[::-1])


def _cached(d1, d2, n, si, pad=(0, 0), new=0):
    return cc._cached(d1, d2, n, si, pad=pad, new=new)


def _pts(*p):
    a = blank_points()
    for k, q in enumerate(p):
        a[k] = q
    return a


def cases():
    cs = []
    K = lambda pos, angle=FLAT, size=(8.0, 2.0): body(CAPSULE, pos, size, angle)      # noqa: E731  (a = 6, r = 2)
    wide, narrow = body(BOX, (0.0, 0.0), (10.0, 3.0)), body(BOX, (0.0, 0.0), (2.0, 3.0))
    # ---- capsule/box ----
    g = "capsule/box"
    cs += scene("kb_flat", g, K((0.0, 4.5)), wide, (2, "end0", "end1"), EXACT, flags=("depth_tie",))
    cs += scene("kb_lean", g, K((0.0, 4.5), 0.05), wide, (2, "end0", "end1"), EVERY)
    cs += scene("kb_lean_back", g, K((0.0, 4.5), -0.05), wide, (2, "end1", "end0"), EVERY)
    cs += scene("kb_on_end", g, K((0.0, 10.5), UP), wide, (1, "end0", None), EVERY)
    cs += scene("kb_on_other_end", g, K((0.0, 10.5), DOWN), wide, (1, "end1", None), EVERY)
    cs += scene("kb_across_tie", g, K((0.5, 4.5)), narrow, (2, "corner2", "corner3"), EXACT, flags=("depth_tie",))
    cs += scene("kb_across", g, K((0.5, 4.5), 0.05), narrow, (2, "corner2", "corner3"), EVERY)
    cs += scene("kb_across_back", g, K((0.5, 4.5), -0.05), narrow, (2, "corner3", "corner2"), EVERY)
    cs += scene("kb_across_under", g, K((0.5, -4.5), 0.05), narrow, (2, "corner1", "corner0"), EVERY)
    cs += scene("kb_half_on", g, K((8.0, 4.5), 0.05), wide, (2, "end0", "corner3"), EVERY)
    cs += scene("kb_half_on_back", g, K((8.0, 4.5), -0.05), wide, (2, "corner3", "end0"), EVERY)
    cs += scene("kb_half_on_tie", g, K((8.0, 4.5)), wide, (2, "end0", "corner3"), EXACT, flags=("depth_tie",))
    cs += scene("kb_corner_clamped", g, K((17.0, 4.0)), wide, (1, "end0", None), EVERY, flags=("clamped:corner3",))
    cs += scene("kb_end_inside", g, K((1.0, 8.0), UP), wide, (1, "end0", None), EVERY, flags=("inside",))
    cs += scene("kb_corner_at_a", g, K((-4.0, 4.5)), narrow, (2, "end1", "corner2"), EXACT, flags=("depth_tie", "at_a", "rejected:corner3:ff"))
    cs += scene("kb_corner_at_minus_a", g, K((4.0, 4.5)), narrow, (2, "end0", "corner3"), EXACT, flags=("depth_tie", "at_a", "rejected:corner2:ff"))
    cs += scene("kb_sep_tie", g, K((0.0, 8.0), UP, (9.0, 3.0)), body(BOX, (0.0, 0.0), (3.0, 3.0)), (2, "end0", "corner2"), EXACT,
                flags=("sep_tie", "inside", "touch"))
    cs += scene("kb_reject_half", g, K((7.525, 7.596), -0.25 * np.pi, (14.0, 8.0)), wide, (1, "corner3", None), EVERY, flags=("rejected:end1:tf",))
    cs += scene("kb_miss", g, K((0.0, 5.5)), wide, (0, None, None), EVERY)
    cs += scene("kb_skewered", g, K((0.0, 0.0), UP), body(BOX, (0.0, 0.0), (2.5, 3.0)), (0, None, None), EVERY, flags=("crossed",))
    # ---- capsule/circle: R = 5 ----
    g = "capsule/circle"
    disc = lambda pos: body(CIRCLE, pos, (3.0, 3.0), 0.6435)      # noqa: E731  (a circle's own frame is never read)
    for name, pos, claim, frames, flags in (("kc_side", (1.0, 4.0), (1, "circle", None), EVERY, ()), ("kc_under", (-2.0, -4.5), (1, "circle", None), EVERY, ()),
                                            ("kc_end", (9.0, 3.0), (1, "circle", None), EVERY, ("at_end",)),
                                            ("kc_other_end", (-9.5, -2.0), (1, "circle", None), EVERY, ("at_end",)),
                                            ("kc_miss", (9.0, 5.0), (0, None, None), EVERY, ()), ("kc_side_miss", (0.0, 5.5), (0, None, None), EVERY, ()),
                                            ("kc_at_a", (6.0, 4.0), (1, "circle", None), EXACT, ("at_a",)), ("kc_at_minus_a", (-6.0, -4.0), (1, "circle", None), EXACT, ("at_a",)),
                                            ("kc_on_core", (2.0, 0.0), (1, "circle", None), EXACT, ("on_core", "crossed")),
                                            ("kc_touch", (0.0, 5.0), (1, "circle", None), EXACT, ("touch",)),
                                            ("kc_touch_end", (9.0, 4.0), (1, "circle", None), EXACT, ("touch", "at_end"))):
        cs += scene(name, g, K((0.0, 0.0)), disc(pos), claim, frames, flags=flags)
    # ---- capsule/capsule: A = {8, 2} (a = 6, r = 2), B = {12, 3} (a = 9, r = 3), R = 5 ----
    g = "capsule/capsule"
    B = lambda pos, angle=FLAT: body(CAPSULE, pos, (12.0, 3.0), angle)      # noqa: E731
    cs += scene("kk_flat", g, K((0.0, 4.5)), B((0.0, 0.0)), (2, "end0", "end1"), EXACT, swapped=(2, "other0", "other1"), flags=("depth_tie",))
    cs += scene("kk_lean", g, K((0.0, 4.5), 0.05), B((0.0, 0.0)), (2, "end0", "end1"), EVERY, swapped=(2, "other0", "other1"))
    cs += scene("kk_lean_back", g, K((0.0, 4.5), -0.05), B((0.0, 0.0)), (2, "end1", "end0"), EVERY, swapped=(2, "other1", "other0"))
    cs += scene("kk_end_to_end", g, K((0.0, 0.0)), B((18.5, 1.0)), (1, "end1", None), EVERY, swapped=(1, "end0", None), flags=("clamped:other0",),
                swapped_flags=("clamped:other1",))
    cs += scene("kk_standing", g, K((2.0, 10.5), UP), B((0.0, 0.0)), (1, "end0", None), EVERY, swapped=(1, "other0", None))
    cs += scene("kk_half_on", g, K((12.0, 4.5), 0.05), B((0.0, 0.0)), (2, "end0", "other1"), EVERY, swapped=(2, "other0", "end1"))
    cs += scene("kk_half_on_back", g, K((12.0, 4.5), -0.05), B((0.0, 0.0)), (2, "other1", "end0"), EVERY, swapped=(2, "end1", "other0"))
    cs += scene("kk_miss", g, K((0.0, 5.5)), B((0.0, 0.0)), (0, None, None), EVERY)
    cs += scene("kk_near_circle", g, K((0.0, 4.5), FLAT, (float(np.nextafter(F(2.0), F(3.0))), 2.0)), B((0.0, 0.0)), (1, "end0", None), EXACT,
                swapped=(1, "other0", None), flags=("near_circle", "depth_tie", "rejected:end1:ff"), swapped_flags=("near_circle", "depth_tie", "rejected:other1:ff"))
    cs += scene("kk_crossed", g, K((0.0, 0.0), FLAT, (5.0, 2.0)), B((0.0, 0.0), UP), (1, "end0", None), EXACT, swapped=(1, "other0", None),
                flags=("crossed", "depth_tie", "rejected:end1:ft"), swapped_flags=("crossed", "depth_tie", "rejected:other1:tf"))
    # ---- the cache: capsule (body 1) flat on the wide box at the scene's origin, as kb_flat without the offset: the new points are
    #      end0 {delta1 (-6, -2), delta2 (-6, 3)} and end1 {delta1 (6, -2), delta2 (6, 3)}, n = (0, 1) ----
    cap, box = record((0.0, 4.5), (8.0, 2.0)), record((0.0, 0.0), (10.0, 3.0))
    near0 = _cached((-5.5, -2.0), (-5.5, 3.0), (1.0, 0.0), 7, pad=(3, 9))
    near1 = _cached((6.5, -2.0), (6.5, 3.0), (1.0, 0.0), 8, pad=(1, 2))
    far = _cached((0.0, -2.0), (0.0, 3.0), (0.0, 1.0), 11)
    far2 = _cached((2.5, -2.0), (2.5, 3.0), (0.0, 1.0), 12, new=1)

    def cache(name, expect, count, pts, b1=cap):
        n = expect[0]
        cs.append(Case(name, "cache", b1, CAPSULE, box, BOX, expect, "end0" if n else None, "end1" if n else None, ("depth_tie",) if n else (), count, pts))
    cache("cache2_matched", (2, (0, 0)), 2, _pts(near0, near1))
    cache("cache2_far", (2, (1, 1)), 1, _pts(far))
    cache("cache2_two_far", (2, (1, 1)), 2, _pts(far, far2))
    cache("cache2_one_matched", (2, (0, 1)), 2, _pts(far, near1))
    cache("cache2_dropped", (0, ()), 2, _pts(near0, far), record((0.0, 9.0), (8.0, 2.0)))
    return cs
