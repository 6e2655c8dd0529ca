"""Directed links: single-step worlds of two or three bodies, each named for what it reaches in tests/link_spec.py (the kind decision,
the activity rule, the clamp, the soft constraint's extremes, the square root's rounding).  tests/test_links_cpu.py proves the claims
on the CPU and holds the spec to the float64 reference (tests/link_reference.py); tests/test_link_corpus_gpu.py runs every case on the
device, byte for byte against the spec.

A case is a LinkMotif: pin_corpus.Motif's bodies (rows, masses, velocities) with links - and pins, where the case is about their
interplay - and the claim `expect` per link: "active", "idle" or "inactive", as link_spec.prestep must find it on the initial state.

Where a case needs an exact length the body sits at the origin with angle 0 (its frame is then exactly the identity), the anchor at
its centre and the other end a world point d: the prestep's d is that point, bit for bit, and len = sqrt(fl(d.x^2) + fl(d.y^2)).
(30, 40) gives len == 50 exactly.

SQRT_D are world points whose float64 sqrt(fl(d.x^2) + fl(d.y^2)) lies within 2^-30 (relative) of the midpoint of two neighbouring
float32 values - a square root that is merely faithful (a bare hardware approximation, 1 ulp) lands on the wrong side of some of
them, a correctly rounded one on the right side of all.  Found by a random search over 1 <= |d.x|, |d.y| <= 90 (about one draw in
fifty qualifies); the figure beside each is its relative distance from the midpoint.  Each is a rod half a unit shorter than its
length, so an ulp of len is an ulp of the bias' leading digits.

ON_A_COMPARISON are the cases whose kind decision sits exactly on a comparison of the prestep (len == max_length, len == min_length,
len == 2^-10).  A float64 reference could decide such a case the other way and would then have to leave it out by name; these are built
from lengths that are exact in either precision (50 = |(30, 40)|, 2^-10), the reference decides them alike, and none is left out."""
import numpy as np

from phyx_amd.api import link_dtype
from pin_corpus import Motif

F = np.float32
DT = 1.0 / 60.0
G = -200.0


def up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def down(x):
    return float(np.nextafter(F(x), F(-np.inf)))


class LinkMotif(Motif):
    def __init__(self, name):
        Motif.__init__(self, name)
        self._links, self.expect = [], []
        self.steps = 2
        self.edit = None                                   # (link, anchors (4,)) applied between step 1 and step 2

    def link(self, a, b, anchor1, anchor2, lo, hi, hertz=0.0, zeta=0.0, impulse=0.0, expect="active"):
        self._links.append((a, b, anchor1, anchor2, lo, hi, hertz, zeta, impulse, 0))
        self.expect.append(expect)
        return len(self._links) - 1

    def link_at(self, a, b, p1, p2, lo, hi, **kw):
        """a link from the world point p1 on body a to the world point p2 on body b (-1: the world)"""
        return self.link(a, b, self.local(a, p1), p2 if b < 0 else self.local(b, p2), lo, hi, **kw)

    @property
    def links(self):
        p = np.zeros(len(self._links), dtype=link_dtype)
        for k, row in enumerate(self._links):
            p[k] = row
        return p

    def unit_graph(self):
        """body1, body2 of the units (the pins, then the links) and the static flags"""
        p, l = self.pins, self.links
        return p["body1"].tolist() + l["body1"].tolist(), p["body2"].tolist() + l["body2"].tolist(), self.is_static().tolist()

    def device_world(self, phyx_amd, gravity=None):
        w = Motif.device_world(self, phyx_amd, gravity)
        got = w.add_links(self.links)
        assert got.tolist() == list(range(len(self._links)))
        return w


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def build(name, tether=False):
    """the case; with `tether` every dynamic body that a link holds also carries a rope to the world that never engages (idle on every
    step, so no arithmetic changes): its component then has two units or more and, under PHX_PIN_GROUP_PINS=1, exceeds the cap - the
    case runs through the trailing group's kernels"""
    m = LinkMotif(name)
    if name.startswith("sqrt_"):
        _sqrt_case(m, SQRT_D[int(name[5:])])
    else:
        CASES[name](m)
    if tether:
        st = m.is_static()
        for i in sorted({b for row in m._links for b in row[:2] if b >= 0 and not st[b]}):
            heavy = i in m.masses and m.masses[i][0] == 0.0               # (no inverse mass and no lever arm: nothing resists)
            m.link(i, -1, (0.0, 0.0), (m.rows[i][0] + 3.0, m.rows[i][1] + 4.0), 0.0, 1.0e6, expect="inactive" if heavy else "idle")
    return m


OUT, IN = (-3.0, -2.0, 0.25), (3.0, 6.0, 0.25)              # moving away from a point up and to the right, and towards it (gravity included)


def _one(m, d, lo, hi, vel=OUT, **kw):
    """one dynamic body at the origin, frame the identity, linked from its centre to the world point d"""
    a = m.body(0.0, 0.0, angle=0.0, vel=vel)
    m.link(a, -1, (0.0, 0.0), d, lo, hi, **kw)


# -- the kind decision, on and beside its comparisons --
@case
def at_max(m):
    """len == max_length: the upper limit is engaged with C = 0"""
    _one(m, (30.0, 40.0), 10.0, 50.0)


@case
def max_one_ulp_inside(m):
    _one(m, (30.0, 40.0), 10.0, up(50.0), impulse=-2.0, expect="idle")


@case
def max_one_ulp_outside(m):
    _one(m, (30.0, 40.0), 10.0, down(50.0))


@case
def at_min(m):
    """len == min_length: the lower limit is engaged with C = 0"""
    _one(m, (30.0, 40.0), 50.0, 90.0, vel=IN)


@case
def min_one_ulp_inside(m):
    _one(m, (30.0, 40.0), down(50.0), 90.0, impulse=2.0, expect="idle")


@case
def min_one_ulp_outside(m):
    _one(m, (30.0, 40.0), up(50.0), 90.0, vel=IN)


@case
def taut_rope(m):
    """a rope (min_length 0) well past its length, moving outwards: the bias and the velocity both pull"""
    a = m.body(0.0, 0.0, angle=0.0, vel=(-6.0, -8.0, 0.0))
    m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 0.0, 48.0)


@case
def rope_moving_inwards(m):
    """past its length but closing faster than the bias asks: the clamp holds the impulse at 0 on every sweep"""
    a = m.body(0.0, 0.0, angle=0.0, vel=(60.0, 80.0, 0.0))
    m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 0.0, 49.9)
    m.gravity = 0.0


# -- the activity rule --
@case
def below_len_floor(m):
    _one(m, (2.0 ** -11, 0.0), 5.0, 5.0, impulse=3.0, expect="inactive")


@case
def at_len_floor(m):
    """len == 2^-10 exactly: not above the floor"""
    _one(m, (0.0, 2.0 ** -10), 5.0, 5.0, impulse=3.0, expect="inactive")


@case
def above_len_floor(m):
    _one(m, (up(2.0 ** -10), 0.0), 1.0, 1.0)


@case
def coincident(m):
    """len == 0: no axis (0 / 0), inactive before anything is made of it"""
    _one(m, (0.0, 0.0), 0.0, 5.0, impulse=-3.0, expect="inactive")


@case
def coincident_bodies(m):
    """two dynamic bodies whose anchors meet in one world point"""
    a, b = m.body(0.0, 0.0, angle=0.0), m.body(8.0, 0.0, angle=0.0)
    m.link(a, b, (4.0, 0.0), (-4.0, 0.0), 2.0, 2.0, impulse=1.0, expect="inactive")


@case
def static_static(m):
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    b = m.body(30.0, 0.0, half=(5.0, 5.0), static=True)
    m.link_at(a, b, (5.0, 0.0), (25.0, 0.0), 10.0, 10.0, impulse=7.0, expect="inactive")


@case
def static_world(m):
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    m.link_at(a, -1, (5.0, 0.0), (25.0, 3.0), 0.0, 10.0, impulse=-7.0, expect="inactive")


@case
def static_end(m):
    """body1 static, body2 dynamic: only body2 is written"""
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    b = m.body(20.0, 3.0)
    m.link_at(a, b, (5.0, 1.0), (18.0, 3.5), 12.0, 12.0)


@case
def axle_off_centre(m):
    """invMass 0, invInertia > 0, linked off-centre across the arm: kinv = iA (ra x n)^2 alone, and the wheel turns"""
    from phyx_amd.api import pinned_inv_inertia
    a = m.body(0.0, 0.0, mass=(0.0, pinned_inv_inertia(3.0, 1.0)), vel=(0.0, 0.0, 0.7))
    m.link_at(a, -1, (2.5, 0.3), (4.0, 9.0), 8.0, 8.0)


@case
def axle_through_centre(m):
    """the same wheel linked at its centre: ra = 0, kinv = 0, nothing resists"""
    from phyx_amd.api import pinned_inv_inertia
    a = m.body(0.0, 0.0, mass=(0.0, pinned_inv_inertia(3.0, 1.0)), vel=(0.0, 0.0, 0.7))
    m.link(a, -1, (0.0, 0.0), (4.0, 9.0), 8.0, 8.0, impulse=1.0, expect="inactive")


@case
def centres(m):
    """anchors at both centres: no lever arm, the rod turns nothing"""
    a, b = m.body(0.0, 0.0, half=(0.5, 0.5)), m.body(12.0, 5.0, half=(0.5, 0.5))
    m.link(a, b, (0.0, 0.0), (0.0, 0.0), 12.0, 12.0)


@case
def rod_pair(m):
    """two rotated dynamic bodies, off-centre anchors, a warm start"""
    a, b = m.body(0.0, 0.0), m.body(14.0, 2.0, half=(4.0, 1.5))
    m.link_at(a, b, (2.5, 0.5), (11.0, 1.0), 9.0, 9.0, impulse=3e-4)


# -- the clamp --
@case
def warm_start_of_the_wrong_sign_upper(m):
    """the upper limit engaged with a stored impulse > 0: the warm start is clamped to 0 before it is applied"""
    a = m.body(0.0, 0.0, angle=0.0, vel=(0.0, 0.0, 0.0))
    m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 0.0, 49.0, impulse=5.0)


@case
def warm_start_of_the_wrong_sign_lower(m):
    a = m.body(0.0, 0.0, angle=0.0, vel=(0.0, 0.0, 0.0))
    m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 51.0, 90.0, impulse=-5.0)


@case
def overflow_after_an_anchor_edit(m):
    """step 1 as a rod at rest length; then the world anchor moves 3e38 away: C (0.2 / dt) overflows, the impulse is inf, the
    velocities inf and NaN (inf n.x with n.y = 0 ...), on the device as in the spec"""
    a = m.body(0.0, 0.0, angle=0.0, vel=(1.0, 0.0, 0.0))
    k = m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 50.0, 50.0)
    m.edit = (k, (0.0, 0.0, 3.0e38, 0.0))


@case
def overflow_on_a_rope(m):
    """the same through the clamp: new = clamp(impulse - inf) = -inf passes lo = -inf, and NaN < lo, NaN > hi are both false"""
    a = m.body(0.0, 0.0, angle=0.0, vel=(1.0, 0.0, 0.0))
    k = m.link(a, -1, (0.0, 0.0), (30.0, 40.0), 0.0, 49.0)
    m.edit = (k, (0.0, 0.0, 3.0e38, 1.0e38))


# -- the soft constraint --
def _spring(m, hertz, zeta):
    a, b = m.body(0.0, 0.0), m.body(14.0, 2.0, half=(4.0, 1.5))
    m.link_at(a, b, (2.5, 0.5), (11.0, 1.0), 6.0, 6.0, hertz=hertz, zeta=zeta)


@case
def spring_1hz(m):
    _spring(m, 1.0, 0.7)


@case
def spring_undamped(m):
    _spring(m, 2.0, 0.0)


@case
def spring_tiny_hertz(m):
    """hertz 1e-3: gamma is huge beside kinv, the spring all but absent"""
    _spring(m, 1.0e-3, 1.0)


@case
def spring_tiny_hertz_undamped(m):
    _spring(m, 1.0e-3, 0.0)


@case
def spring_huge_hertz(m):
    """hertz 1e4, far above the step rate: gamma vanishes beside kinv and bias tends to C / dt, five times the rod's"""
    _spring(m, 1.0e4, 1.0)


@case
def spring_to_the_world(m):
    a = m.body(0.0, 0.0)
    m.link_at(a, -1, (2.0, 0.5), (9.0, 12.0), 4.0, 4.0, hertz=3.0, zeta=0.5, impulse=-2e-4)


# -- among other units --
@case
def rope_on_a_pinned_body(m):
    """a pin and a taut rope on one body: two units in two classes, one sweep over both"""
    a = m.body(0.0, 0.0)
    m.pin_at(a, -1, (-3.0, 0.0), flags=(True, True, False))
    m.link_at(a, -1, (3.0, 0.0), (3.0, 21.0), 0.0, 20.0)


@case
def rod_rope_pin(m):
    """three bodies: a rod, a rope past its length and a pin in a row"""
    a, b, c = m.body(0.0, 0.0), m.body(12.0, 0.0), m.body(24.0, 0.0)
    m.link_at(a, b, (2.0, 0.0), (10.0, 0.5), 8.0, 8.0)
    m.link_at(b, c, (14.0, 0.0), (22.0, -0.5), 0.0, 7.5)
    m.pin_at(c, -1, (27.0, 0.0), flags=(True, True, False))


# -- the square root --
SQRT_D = (
    (65.94232940673828, 13.888389587402344),      # 5.6e-10
    (-9.54119873046875, -18.864852905273438),     # 1.2e-10
    (-62.19602584838867, -60.39041519165039),     # 7.1e-10
    (-85.54161071777344, 65.03227233886719),      # 2.2e-10
    (-62.79069519042969, 34.17948532104492),      # 7.7e-10
    (-4.305944442749023, -55.62861251831055),     # 6.4e-10
    (72.51909637451172, -69.65802764892578),      # 5.5e-10
    (44.24845886230469, -59.90836715698242),      # 8.7e-10
    (61.53495788574219, 87.6585464477539),        # 5.5e-10
    (34.976593017578125, -69.87179565429688),     # 6e-10
    (69.06097412109375, -14.184598922729492),     # 4.6e-10
    (26.903682708740234, 53.47761917114258),      # 6.8e-10
    (-6.562823295593262, 55.32426834106445),      # 9.1e-10
    (44.27651596069336, -88.45881652832031),      # 7.8e-11
    (-72.14511108398438, -28.522459030151367),    # 3.8e-10
    (-82.71607208251953, 63.952117919921875),     # 3.9e-10
    (46.225521087646484, 5.460998058319092),      # 7.1e-11
    (-38.47819900512695, -45.622337341308594),    # 7.7e-10
    (5.730409622192383, 29.97105598449707),       # 3.2e-10
    (-68.43838500976562, 30.437467575073242),     # 1.9e-10
    (18.314828872680664, -45.84376907348633),     # 2.9e-10
    (61.29909133911133, 9.153097152709961),       # 5.2e-10
    (-10.109186172485352, -82.73291778564453),    # 2e-10
    (-33.622467041015625, 41.23291015625),        # 2.4e-10
)


def sqrt_midpoint_distance(d):
    """the relative distance of the float64 sqrt(fl(d.x^2) + fl(d.y^2)) from the nearest midpoint of two float32 neighbours"""
    x, y = F(d[0]), F(d[1])
    s = F(x * x) + F(y * y)
    r = np.sqrt(np.float64(s))
    near = F(r)
    mids = [(np.float64(near) + np.float64(np.nextafter(near, F(t)))) / 2.0 for t in (np.inf, -np.inf)]
    return min(abs(r - mid) for mid in mids) / r


def _sqrt_case(m, d):
    x, y = F(d[0]), F(d[1])
    ln = float(np.sqrt(F(x * x) + F(y * y)))
    _one(m, (float(x), float(y)), ln - 0.5, ln - 0.5, vel=(0.0, 0.0, 0.0))
    m.gravity = 0.0                                         # (the impulse is the bias' alone: C = len - L to its last digit)


NAMES = tuple(CASES) + tuple("sqrt_%d" % k for k in range(len(SQRT_D)))
ON_A_COMPARISON = ("at_max", "at_min", "at_len_floor")
NON_FINITE = ("overflow_after_an_anchor_edit", "overflow_on_a_rope")


def state_of(w):
    """a link's prestep record as the cases' `expect` names it"""
    return "active" if w.active else ("idle" if w.idle else "inactive")
