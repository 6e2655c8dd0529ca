"""A directed corpus for the round queries at the scale of the project's worlds (tests/round_query_reference.py is its judge), in the
manner of tests/query_corpus.py, whose body sets and conventions (NEAR, CAP, DESIGN, DISTANCES, LENGTHS, BOUND) it uses: query circles
and circle casts placed against each body by construction.

What varies: query radii 1e-3 .. 100 (RADII, taken in turn), the distance of a cast's origin from the body it is aimed at (1 .. 10^6
units), the distance of the bodies from the world's origin (3000, 10^5), circle bodies of radius 0.5 .. 8 and one of 500 (r + rb from 0.5
to 600), boxes at angles that include 0 and pi / 2 exactly, direction lengths 1e-3, 1 and 1e3, the line through the centre and at 0.5
and 0.9 of the widened body's half width, past it at 1.5, and casts that start overlapping.  Circles are placed in a box's frame: the
centre inside, beside each of the four faces and in each of the four corner regions, at 0.5 and 0.9 of the radius from the surface
(overlapping) and at 1.5 (clear).  The directed casts are laid out in a box's frame too, so that each of the six parts of the rule wins:
the wide box through its x axis, the tall box through its y axis, along an axis with the other local component exactly zero (the exact
frames), and every corner disc entered from both of its sides.

A case's `circles` and `casts` are the ones whose verdict is clear BY DESIGN: a query is generated only where the designed clearance is
at least DESIGN u, u = 2^-24 * the largest coordinate or size involved, so that the judge's excused share stays under CAP whatever the
code under test does.  `near_circles` and `near_casts` are the deliberately doubtful ones: tangent at 0.999 and 1.001 of the clearance,
max_t one ulp short of, at and one ulp past the entry.  They are only asserted to be excused or right."""
import functools

import numpy as np

import query_corpus as qc
import round_query_reference as ref
from query_corpus import BOX, CIRCLE, CAP, DESIGN, DISTANCES, LENGTHS, NEAR, judged, records, world      # noqa: F401  (the tests take them from here)

F = np.float32
RADII = (1e-3, 0.5, 3.0, 100.0)
# Every measure of a hit both sides agree on, in u.  query_corpus.BOUND (16 u: a rule is a chain of about a dozen float32 operations on
# quantities no larger than scale) holds for a circle body's three measures and for a box's length: the specification's worst on the
# asserted casts is disc hit 2.59, normal 2.65, length 1.71, box length 2.07.  A box's `hit` keeps query_corpus.BOUNDS[("box", "hit")]
# (64 u), the grazing-angle term: the surface is met at the angle phi, and what the roundings of o' (the origin in the body's frame, a
# few u of the world's scale, not of the part's size) move the entry by along the cast is 1 / sin(phi) times their size, through a
# face of the wide or the tall box as for a ray, and through a corner's arc as well: the arc of a large circle around a small box is
# met at a shallow angle long before the cast as a whole grazes.  The corpus has arcs entered at sin(phi) = 0.088 (1 / sin = 11.3:
# r = 100 against the 7 x 4 box, the line at 0.9 of the widened half width); the worst measured there is 39.6 u.  A box's `normal`
# has the same term, which a ray's never had (a ray's box normal is a stored axis): on an arc the normal turns with the entry point,
# so as a length on the arc's radius its error is the hit's, seen across the cast: 35.8 u at the same cast.  128 is the smallest power
# of two that holds with a factor 2 to spare.
# What this admits as an angle: `normal` is the angle times rho (round_query_reference), so a limit of L u admits L * u / rho
# radians.  Around a corner rho = r, and a cast is asserted only where r >= DESIGN u: at the smallest radius, 1e-3, that is 128 u / r,
# 7.6e-3 rad beside a body near the origin (scale 1, u = 6e-8) and up to 128 / 64 = 2 rad where the radius is barely resolved
# (scale 260, the largest at which 1e-3 is still asserted); measured on the body's size instead, as a ray's is, the same limit
# would admit 1000 times less at r = 1e-3 against a body of size 1, which no rule meets, and 100 times more at r = 100.  The
# specification's worst angle around a corner at r = 1e-3 is 6.1e-3 rad (2.3 u of r, "parts"); at 0.5, 3 and 100 it is 2.7e-3,
# 1.3e-2 (from 10^6 away) and 7.5e-4 rad, all under 1.3 u on r.
BOUND = qc.BOUND
BOUNDS = {("box", "hit"): qc.BOUNDS[("box", "hit")], ("box", "normal"): 128.0}
DIRECTIONS = (0.0, float(np.arctan2(0.6, 0.8)), 7.0 * np.pi / 6.0)
FRACTIONS = (0.0, 0.5, -0.9, 1.5)
GRAZE = (0.999, -1.001)


class Case:
    def __init__(self, name, rows):
        self.name, self.rows = name, rows
        self.bodies, self.kinds = records(rows)
        self.circles, self.near_circles, self.casts, self.near_casts = [], [], [], []

    def done(self):
        for k, width in (("circles", 3), ("near_circles", 3), ("casts", 6), ("near_casts", 6)):
            setattr(self, k, np.array(getattr(self, k), dtype=F).reshape(-1, width))
        return self


def _u(*lengths):
    return 2.0 ** -24 * max(1.0, *lengths)


def _one(row):
    b, k = records([row])
    return ref.Bodies(b, k)


def _widths(B, e, r):
    """(half width across e, reach along e) of the one body of B widened by r, for the unit direction e."""
    if B.round[0]:
        return B.rb[0] + r, B.rb[0] + r
    p = np.array([-e[1], e[0]])
    across = abs(B.xv[0] @ p) * B.h[0, 0] + abs(B.yv[0] @ p) * B.h[0, 1]
    along = abs(B.xv[0] @ e) * B.h[0, 0] + abs(B.yv[0] @ e) * B.h[0, 1]
    return across + r, along + r


def _aimed(c, w, reach, e, f, dist, length, r):
    """The cast along e whose line passes the centre c at f * w, starting dist before the widened body; d = e * length."""
    p = np.array([-e[1], e[0]])
    o = c - (dist + reach) * e + f * w * p
    return [o[0], o[1], r, e[0] * length, e[1] * length, 2.0 * (dist + 2.0 * reach) / length + 1.0]


def _beside(A, o, e, r):
    """How far, in length, the line through o along the unit direction e is from grazing each body of A widened by r."""
    p = np.array([-e[1], e[0]])
    across = np.where(A.round, A.rb, np.abs(A.xv @ p) * A.h[:, 0] + np.abs(A.yv @ p) * A.h[:, 1]) + r
    return np.abs(np.abs((A.pos - o) @ p) - across)


def add_casts(case, dist):
    """Casts at every body of the case from `dist`, in every direction, at every fraction that is clear by design, the radius and the
    direction's length taken in turn; the grazing ones and the max_t ones go to near_casts."""
    n = 0
    A = ref.Bodies(case.bodies, case.kinds)
    for row in case.rows:
        B = _one(row)
        for th in DIRECTIONS:
            e = np.array([np.cos(th), np.sin(th)])
            r, length = RADII[n % 4], LENGTHS[n % 3]
            n += 1
            w, reach = _widths(B, e, r)
            u = _u(dist + reach + np.hypot(*B.pos[0]), w, reach)
            for f in FRACTIONS:
                c = _aimed(B.pos[0], w, reach, e, f, dist, length, r)
                if w * abs(1.0 - abs(f)) >= DESIGN * u:                 # (a line that happens to graze another body of the set is doubtful too)
                    (case.casts if (_beside(A, np.array(c[:2]), e, r) >= DESIGN * u).all() else case.near_casts).append(c)
            for f in GRAZE:
                case.near_casts.append(_aimed(B.pos[0], w, reach, e, f, dist, length, r))
            if th == DIRECTIONS[1] and w * 0.5 >= DESIGN * u:           # max_t at the entry, one ulp short of it and one beyond
                c = _aimed(B.pos[0], w, reach, e, 0.5, dist, length, r)
                t = F(ref.cast(B, c).t[0])
                case.near_casts += [c[:5] + [m] for m in (np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf)))]
                short = min(reach, 0.5 * dist)
                if short >= DESIGN * u:
                    case.casts.append(c[:5] + [float(t) - short / length])      # well short of the body: a clear miss
        inner = min(row[3], row[4])
        if 0.5 * inner >= DESIGN * _u(np.hypot(*B.pos[0]), row[3], row[4]):       # the cast starts overlapping: the centre inside, and within r outside
            c = B.pos[0]
            case.casts += [[c[0] + 0.3 * inner, c[1] - 0.2 * inner, RADII[n % 4], 0.6, 0.8, 10.0], [c[0], c[1], 0.5, -1e-3, 2e-3, 1.0]]
    return case


def _frame(B, a, b):
    """The world point (or, for a direction, vector + pos) at the local coordinates (a, b) of the one body of B."""
    return B.pos[0] + a * B.xv[0] + b * B.yv[0]


REGIONS = tuple((sx, sy) for sy in (-1, 0, 1) for sx in (-1, 0, 1) if (sx, sy) != (0, 0))      # the four faces and the four corners


def add_circles(case):
    """Circles at every body: the centre inside; for a box beside each face and in each corner region, for a disc around it; at 0.5, 0.9
    and 1.5 of the radius from the surface, tangent ones (0.999, 1.001) to near_circles.  The radius is taken in turn."""
    n = 0
    for row in case.rows:
        B = _one(row)
        h, pos = B.h[0], B.pos[0]
        case.circles.append([*_frame(B, 0.3 * h[0], -0.2 * h[1]), RADII[n % 4]] if not B.round[0] else [pos[0] + 0.3 * h[0], pos[1], RADII[n % 4]])
        for k, (sx, sy) in enumerate(REGIONS):
            r = RADII[n % 4]
            n += 1
            u = _u(np.hypot(*pos) + h.max() + 2.0 * r, h.max(), r)
            for f in (0.5, 0.9, 1.5, 0.999, 1.001):
                gap = f * r
                if B.round[0]:
                    e = np.array([sx, sy]) / np.hypot(sx, sy)
                    c = pos + (B.rb[0] + gap) * e
                elif sx and sy:                                         # a corner region, off the diagonal
                    c = _frame(B, sx * (h[0] + gap * 0.8), sy * (h[1] + gap * 0.6))
                else:                                                   # a face region, off the middle
                    c = _frame(B, sx * (h[0] + gap) + (0.6 * h[0] if sy else 0.0) * (1 if k % 2 else -1),
                               sy * (h[1] + gap) + (0.6 * h[1] if sx else 0.0) * (1 if k % 2 else -1))
                if f in (0.999, 1.001):
                    case.near_circles.append([c[0], c[1], r])
                elif r * abs(1.0 - f) >= DESIGN * u:
                    case.circles.append([c[0], c[1], r])
    return case


def add_directed(case, dist=30.0):
    """Casts laid out in each box's frame so that every part wins: along +x at 0.3 h.y (the wide box through x; in an exact frame d'.y is
    exactly 0), along -y at -0.4 h.x (the tall box through y; d'.x exactly 0), and at every corner along the line through the box's
    corner at 0.3 rad from either of its two faces (the corner's disc, entered from both sides).  A disc body gets the two axis casts."""
    n = 0
    for row in case.rows:
        B = _one(row)
        h, pos = B.h[0], B.pos[0]
        for k in range(2 if B.round[0] else 10):
            r, length = RADII[n % 4], LENGTHS[n % 3]
            n += 1
            if r < DESIGN * _u(np.hypot(*pos) + dist + h.max() + r, h.max(), r):
                continue
            if k == 0:
                at, dl = (-(h[0] + r + dist), 0.3 * h[1]), (1.0, 0.0)
            elif k == 1:
                at, dl = (-0.4 * h[0], h[1] + r + dist), (0.0, -1.0)
            else:
                sx, sy = ((-1, -1), (1, -1), (-1, 1), (1, 1))[(k - 2) // 2]
                al = 0.3 if k % 2 == 0 else np.pi / 2 - 0.3
                out = np.array([sx * np.cos(al), sy * np.sin(al)])      # from the corner outwards
                at, dl = np.array([sx * h[0], sy * h[1]]) + (r + dist) * out, -out
            o = _frame(B, at[0], at[1])
            d = (dl[0] * B.xv[0] + dl[1] * B.yv[0]) * length
            case.casts.append([o[0], o[1], r, d[0], d[1], 2.0 * (dist + 2.0 * (h.max() + r)) / length])
    return case


@functools.lru_cache(maxsize=None)
def cases():
    """The corpus, built once per process; the tests leave it unchanged."""
    out = []
    for dist in DISTANCES:
        out.append(add_casts(Case("from %g" % dist, qc.small_set()), dist).done())
    out.append(add_circles(add_directed(Case("parts", qc.small_set()))).done())
    out.append(add_circles(add_casts(add_casts(Case("big disc", qc.big_set()), 30.0), 1e6)).done())
    for name, shift in (("bodies at 3000", (3000.0, -3000.0)), ("bodies at -1e5", (-1e5, 1e5))):
        out.append(add_circles(add_directed(add_casts(Case(name, qc.small_set(shift)), 30.0))).done())
    row = Case("a row of discs from 3000", qc.row_set())
    for y in (0.0, 0.5, -0.9, 1.3):                                     # (1.3: past the first discs of radius 1, r + rb = 1.25, into a larger one)
        row.casts += [[-3000.0, y, 0.25, 1.0, 0.0, 4000.0], [3030.0, y, 0.25, -1e3, 0.0, 4.0], [-3000.0, y, 0.25, 1.0, 0.0, 2990.0]]
    out.append(row.done())
    many = qc.small_set() + qc.small_set((3000.0, 700.0)) + qc.small_set((-3000.0, 700.0)) + qc.small_set((0.0, 3000.0)) + qc.row_set(-3000.0)[:5]
    assert len(many) == 65
    out.append(add_directed(Case("65 bodies", many), 300.0).done())
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def boxes_only(c):
    """The case's boxes alone, as a world without a shape column has them: (records, None)."""
    return c.bodies[c.kinds == BOX], None


def assert_bounds(worst, what):
    for (kind, m), (figure, q) in worst.items():
        bound = BOUNDS.get((kind, m), BOUND)
        assert figure <= bound, "%s: %s %s is %.3g u at cast %d, the bound is %g u" % (what, kind, m, figure, q, bound)


def table(worst):
    return "  ".join("%s %s" % (kind, " ".join("%s %.3g" % (m, worst[(kind, m)][0]) for m in ref.MEASURES)) for kind in ("box", "disc"))


# ---- an answer held to the judge --------------------------------------------------------------------------------------------------------
def judge_casts(bodies, kinds, casts, got, verdicts=None):
    """cast_circles' answer `got` (shape_hit_dtype) for `casts` against the judge, as query_corpus.judge_hits.  A (cast, body) pair is
    doubtful when the body's clearance is within NEAR u; a cast is doubtful when some pair of it is, or two bodies' entries lie within
    NEAR u of each other at the front.  Every other cast must name the judge's closest body, with a normal of (0, 0) exactly when the
    judge has the cast start overlapping.  Where the named body is one the judge sees hit, the deviation() measures are collected
    whether the cast is doubtful or not, except `hit` of a pair that is.  A doubtful cast is only held to naming a body the judge sees
    hit, or one within NEAR u of it, and to no hit only when every hit the judge sees is that close.  verdicts(c) -> (N,) bool, the
    rule's own verdict on every body, equals the judge's on every pair that is not doubtful.
    Returns (doubtful pairs (K, N) bool, worst {("box" | "disc", measure): (figure in u, cast index)})."""
    B = ref.Bodies(bodies, kinds)
    pairs = np.zeros((len(casts), B.n), dtype=bool)
    worst = {(k, m): (0.0, -1) for k in ("box", "disc") for m in ref.MEASURES}
    for q, c in enumerate(casts):
        v = ref.cast(B, c)
        u = ref.unit(B, c, v)
        dlen = float(np.hypot(np.float64(F(c[3])), np.float64(F(c[4]))))
        close = v.clearance <= NEAR * u
        pairs[q] = close
        want = ref.closest(v)
        front = np.where(v.hit, v.t, np.inf) * dlen
        rivals = np.zeros(B.n, dtype=bool)
        if want >= 0:
            rivals = (front <= front[want] + NEAR * u) & v.hit
            rivals[want] = False
        doubtful = close.any() or rivals.any()
        if verdicts is not None:
            wrong = (np.asarray(verdicts(c), dtype=bool) != v.hit) & ~close
            assert not wrong.any(), "cast %d %s: bodies %s, the judge says hit = %s, clear by %s u" % (q, c, np.flatnonzero(wrong), v.hit[wrong], (v.clearance / u)[wrong])
        b = int(got["body"][q])
        if not doubtful:
            assert b == want, "cast %d %s: body %d, the judge has %d" % (q, c, b, want)
        elif b >= 0:
            assert v.hit[b] or close[b], "cast %d %s: body %d, which the judge sees missed by %g u" % (q, c, b, v.clearance[b] / u[b])
        else:
            assert not (v.hit & ~close).any(), "cast %d %s: no hit, the judge has body %d clear by %g u" % (q, c, want, v.clearance[want] / u[want])
        if b < 0 or not v.hit[b]:
            continue
        normal = (float(got["normal"][q][0]), float(got["normal"][q][1]))
        if not close[b]:
            assert (normal == (0.0, 0.0)) == bool(v.inside[b]), "cast %d %s: normal %s, inside %s" % (q, c, normal, v.inside[b])
        if normal == (0.0, 0.0):
            v.normal[b] = np.nan
        dev = ref.deviation(B, c, v, b, got["t"][q], normal)
        for m in ref.MEASURES:
            if close[b] and m == "hit":
                continue
            key = ("disc" if B.round[b] else "box", m)
            if dev[m] / u[b] > worst[key][0]:
                worst[key] = (dev[m] / u[b], q)
    return pairs, worst


def judge_circles(bodies, kinds, circles, offsets, hits):
    """query_circles' answer against the judge: every (circle, body) pair whose clearance exceeds NEAR u is listed exactly when the judge
    sees an overlap.  Returns the doubtful pairs (K, N) bool."""
    B = ref.Bodies(bodies, kinds)
    pairs = np.zeros((len(circles), B.n), dtype=bool)
    for q, c in enumerate(circles):
        hit, clear = ref.overlap(B, c)
        pairs[q] = clear <= NEAR * ref.unit(B, c)
        mine = np.zeros(B.n, dtype=bool)
        mine[hits[offsets[q]:offsets[q + 1]]] = True
        wrong = (mine != hit) & ~pairs[q]
        assert not wrong.any(), "circle %d %s: bodies %s, the judge says overlap = %s, clear by %s u" % (
            q, c, np.flatnonzero(wrong), hit[wrong], (clear / ref.unit(B, c))[wrong])
    return pairs
