"""The directed corpus of the continuous bodies' pass (include/phyx_amd.h CONTINUOUS BODIES): small worlds of a few static targets and
one swept body each, built so that over the corpus the specification (tests/sweep_spec.py) takes every arm it has:
  per target kind   every part or candidate as the winner: a box's two widened boxes and four corner discs, a circle body, a capsule's
                    two sides and two ends, every face and every vertex of a triangle and of an 8-gon, each at three placements;
  between targets   a tie of two targets, won by the lower index; a filtered, a sensor and an excluded target in front of a real one;
                    a sleeper (both inverse masses read 0) as a target;
  the arms          a start that overlaps, a touch that does not approach, a step that creeps in by less than the skin and one just
                    faster, a fast step from a skin short of the touch (held at t' = 0), d = 0, t exactly 0 and t exactly 1;
  polygons passed   a triangle and an 8-gon passed, left and not reached, beside their faces where the faces' planes reach far outside.
A case holds its targets (bodies 0 .. m-1) and its swept body (body m, a circle of radius 0.5 with the core radius 0.4): the records
behind IntegratePosition (the swept body at e = s + d), the start s, and what the specification is expected to answer.  ILL names the
cases the float64 judge cannot be asked about: a grazing touch, and the start and the end that lie on the outline to a rounding.
RULE_ONLY names the case that shows the rule's own exception, which the judge does not know: tests/test_sweep_cpu.py holds it to a
stated expectation instead."""
import numpy as np

import polygon_spec as ps
import query_corpus as qc

F = np.float32
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
RC, R = 0.4, 0.5                        # the swept body: a circle of radius R, core radius RC (factor 0.8)
DT = 1.0 / 64.0                         # the lockstep's time step: d = v * DT is exact for v = 64 d
TRIANGLE = ps.polygon([(-2.0, -1.0), (2.0, -1.0), (0.0, 2.0)])
OCTAGON = ps.regular(8, 2.0, np.pi / 8)
PLACEMENTS = ((0.0, 0.0, "0"), (3.0, -1.5, 0.7), (-40.0, 25.0, 2.4))      # (px, py, angle) of a directed target; "0": the exact frame
ILL = ("graze-no-approach", "t-exactly-0", "t-exactly-1")
RULE_ONLY = ("creeping-in",)            # the rule's own exception, which the judge does not know: tested against stated expectations


class Case:
    def __init__(self, name, targets, s, d, want, polys=None, flags=None, filters=None, exclusions=None, rc=RC, r=R):
        """targets: rows (px, py, angle, hx, hy, kind); s, d: the swept body's start and translation; rc, r: its core radius and its own;
        want: (target or None, label; a label of None beside a target: not looked at)."""
        self.name, self.want, self.rc_value = name, want, rc
        m = len(targets)
        s = np.asarray(s, dtype=F)
        e = (s + np.asarray(d, dtype=F)).astype(F)
        rows = list(targets) + [(float(e[0]), float(e[1]), "0", r, r, CIRCLE)]
        self.bodies, self.kinds = qc.records(rows)
        self.bodies["inv_mass"][:m] = 0
        self.bodies["inv_inertia"][:m] = 0
        self.polys = [ps.NONE] * (m + 1) if polys is None else list(polys) + [ps.NONE]
        self.start = np.zeros((m + 1, 2), dtype=F)
        self.start[:m, 0], self.start[:m, 1] = self.bodies["pos"]["x"][:m], self.bodies["pos"]["y"][:m]
        self.start[m] = s
        self.rc = np.zeros(m + 1, dtype=F)
        self.rc[m] = rc
        self.flags, self.filters, self.exclusions = flags, filters, exclusions
        self.mover = m


def _world(place, p):
    """The frame point p of a target placed at `place`, in the world (float64; the case rounds it to float32)."""
    px, py, ang = place
    a = 0.0 if isinstance(ang, str) else ang
    c, s = np.cos(a), np.sin(a)
    return np.array([px + c * p[0] - s * p[1], py + s * p[0] + c * p[1]])


def _turn(place, v):
    return _world((0.0, 0.0, place[2]), v)


def _poly_row(place, poly):
    hx, hy = ps.frame_box(poly)
    return (place[0], place[1], place[2], float(hx), float(hy), POLYGON)


def _directed():
    out = []
    for pi, place in enumerate(PLACEMENTS):
        tag = "@%d" % pi
        # a box {2, 1}: the x face (the wide box), the y face (the tall box), the four corner discs (-,-) (+,-) (-,+) (+,+)
        box = (place[0], place[1], place[2], 2.0, 1.0, BOX)
        aims = [((0, "x"), (-4.0, 0.3), (2.5, 0.0)), ((1, "y"), (0.6, 3.0), (0.0, -2.5))]
        aims += [(2 + k, (sx * 3.2, sy * 2.2), (-sx * 1.5, -sy * 1.5)) for k, (sx, sy) in enumerate(((-1, -1), (1, -1), (-1, 1), (1, 1)))]
        for label, o, d in aims:
            out.append(Case("box-%s%s" % (label, tag), [box], _world(place, o), _turn(place, d), (0, label)))
        # a circle body of radius 1
        out.append(Case("circle%s" % tag, [(place[0], place[1], place[2], 1.0, 1.0, CIRCLE)], _world(place, (-2.5, 0.4)), _turn(place, (2.0, 0.0)), (0, 6)))
        # a capsule {2, 0.75}: both sides, both ends
        cap = (place[0], place[1], place[2], 2.0, 0.75, CAPSULE)
        for label, o, d in (("side+", (0.3, 2.5), (0.0, -2.0)), ("side-", (-0.3, -2.5), (0.0, 2.0)), ("end0", (-4.0, 0.2), (2.0, 0.0)), ("end1", (4.0, -0.2), (-2.0, 0.0))):
            out.append(Case("capsule-%s%s" % (label, tag), [cap], _world(place, o), _turn(place, d), (0, label)))
        # a triangle and an 8-gon: every face from along its normal, every vertex from along its direction from the origin
        for name, poly in (("triangle", TRIANGLE), ("octagon", OCTAGON)):
            count = int(poly["count"])
            v = np.asarray(poly["v"], dtype=np.float64)[:count]
            n = ps.normals(count, poly["v"]).astype(np.float64)[:count]
            for k in range(count):
                mid = 0.55 * v[k] + 0.45 * v[(k + 1) % count]
                out.append(Case("%s-face%d%s" % (name, k, tag), [_poly_row(place, poly)], _world(place, mid + n[k] * 2.0), _turn(place, -n[k] * 1.9), (0, ("face", k)), polys=[poly]))
                u = v[k] / np.hypot(*v[k])
                out.append(Case("%s-vertex%d%s" % (name, k, tag), [_poly_row(place, poly)], _world(place, v[k] + u * 2.0), _turn(place, -u * 1.9), (0, ("vertex", k)), polys=[poly]))
    return out


def _filters(m, blocked):
    """Default filters for m + 1 bodies, body `blocked` in a category the swept body's mask leaves out."""
    import filter_spec
    f = filter_spec.filters(m + 1)
    f["category"][blocked] = 2
    f["mask"][m] = 0xFFFFFFFF & ~2
    return f


def _arms():
    box = (0.0, 0.0, "0", 1.0, 1.0, BOX)                                    # an exact frame: the faces at +-1, widened by RC to +-1.4
    front = (-1.5, 0.0, "0", 0.25, 1.0, BOX)                                # a thin wall in front of `back`
    back = (1.0, 0.0, "0", 1.0, 1.0, BOX)
    s, d = (-4.0, 0.25), (4.0, 0.0)
    tri = (6.0, 0.0, 0.0, 2.0, 2.0, POLYGON)
    tri0, oct0 = (0.0, 0.0, 0.0, 2.0, 2.0, POLYGON), _poly_row((0.0, 0.0, 0.0), OCTAGON)
    flags = np.zeros(3, dtype=np.uint32)
    flags[0] = 1
    return [
        Case("tie-by-index", [box, box], (-3.0, 0.5), (2.0, 0.0), (0, (0, "x"))),
        Case("tie-by-index-polygon", [_poly_row((0.0, 0.0, 0.3), OCTAGON)] * 2, (-4.0, 0.1), (3.0, 0.0), (0, None), polys=[OCTAGON, OCTAGON]),
        Case("nearer-wins", [back, front], s, d, (1, (0, "x"))),
        Case("filtered-in-front", [front, back], s, d, (1, (0, "x")), filters=_filters(2, 0)),
        Case("sensor-in-front", [front, back], s, d, (1, (0, "x")), flags=flags),
        Case("excluded-in-front", [front, back], s, d, (1, (0, "x")), exclusions=np.array([[2, 0]], dtype=np.int32)),
        Case("sensor-swept", [front, back], s, d, (None, None), flags=np.array([0, 0, 1], dtype=np.uint32)),
        Case("sleeper-target", [box], (-3.0, 0.0), (2.5, 0.0), (0, (0, "x"))),      # (a sleeper's inverse masses read 0: the records say no more)
        Case("start-overlap-box", [box], (-1.2, 0.0), (1.0, 0.0), (None, "overlap")),
        Case("start-overlap-circle", [(0.0, 0.0, "0", 1.0, 1.0, CIRCLE)], (-1.3, 0.0), (1.0, 0.0), (None, "overlap")),
        Case("start-overlap-capsule", [(0.0, 0.0, "0", 2.0, 0.75, CAPSULE)], (0.0, 1.0), (0.0, -1.0), (None, "overlap")),
        Case("start-overlap-polygon-face", [tri], (6.0, -1.3), (0.0, 1.0), (None, "overlap"), polys=[TRIANGLE]),
        Case("start-overlap-polygon-vertex", [tri], (6.0, 2.3), (0.0, -1.0), (None, "overlap"), polys=[TRIANGLE]),
        Case("start-inside-polygon", [tri], (6.0, 0.0), (0.0, 3.0), (None, "overlap"), polys=[TRIANGLE]),
        Case("overlap-in-front-of-a-real-one", [front, back], (-1.9, 0.0), (2.0, 0.0), (1, (0, "x"))),
        Case("moving-away", [box], (-3.0, 0.0), (-2.0, 0.0), (None, None)),
        Case("short-of-it", [box], (-4.0, 0.0), (2.0, 0.0), (None, None)),
        Case("beside-it", [box], (-4.0, 3.0), (8.0, 0.0), (None, None)),
        Case("d-is-zero", [box], (-1.6, 0.0), (0.0, 0.0), (None, None)),
        Case("graze-no-approach", [box], (-1.5, -3.0), (0.0, 2.0), (None, "away"), rc=0.5, r=1.0),
        Case("t-exactly-0", [box], (-1.5, 0.0), (0.5, 0.0), (0, (0, "x")), rc=0.5, r=1.0),
        Case("held-a-skin-short", [box], (-1.5 - 0.0078125, 0.0), (0.5, 0.0), (0, (0, "x")), rc=0.5, r=1.0),      # (the skin of rc 0.5 is 0.0078125: t' = 0)
        Case("creeping-in", [box], (-1.504, 0.0), (0.006, 0.3), (None, "away"), rc=0.5, r=1.0),
        Case("just-faster-than-creeping", [box], (-1.504, 0.0), (0.009, 0.3), (0, (0, "x")), rc=0.5, r=1.0),
        # a polygon passed, left and not reached: the pushed-out planes of its faces reach far outside it
        Case("triangle-beside-the-slope-leaving", [tri0], (1.5, 1.5), (0.5, 1.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-beside-the-other-slope-leaving", [tri0], (-1.5, 1.5), (0.5, 1.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-off-the-slope-leaving", [tri0], (1.9, 1.9), (0.5, 1.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-moving-away", [tri0], (0.0, -2.0), (0.0, -2.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-short-of-it", [tri0], (-5.0, 0.0), (2.0, 0.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-beside-it", [tri0], (-5.0, 3.0), (10.0, 0.0), (None, None), polys=[TRIANGLE]),
        Case("triangle-past-its-vertex", [tri0], (-3.0, 2.6), (6.0, 0.0), (None, None), polys=[TRIANGLE]),
        Case("octagon-moving-away", [oct0], (2.6, 0.5), (1.5, 0.5), (None, None), polys=[OCTAGON]),
        Case("octagon-short-of-it", [oct0], (-5.0, 0.3), (2.0, 0.0), (None, None), polys=[OCTAGON]),
        Case("octagon-beside-it", [oct0], (-5.0, 2.6), (10.0, 0.0), (None, None), polys=[OCTAGON]),
        Case("octagon-along-a-face-leaving", [oct0], (2.45, -0.5), (0.3, 2.0), (None, None), polys=[OCTAGON]),
        Case("t-exactly-1", [box], (-2.5, 0.25), (1.0, 0.0), (0, (0, "x")), rc=0.5, r=1.0),
    ]


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _directed() + _arms()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)
