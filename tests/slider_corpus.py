"""Directed sliders: single-step worlds of one or two bodies, each named for what it reaches in tests/slider_spec.py (the geometry's
special places, the activity rule, the limit decision on and beside its comparisons, the clamps, the three rows together).
tests/test_sliders_cpu.py proves the claims on the CPU and holds the spec to the float64 reference (tests/slider_reference.py);
tests/test_slider_corpus_gpu.py runs every case on the device, byte for byte against the spec.

A case is a SliderMotif: angle_corpus.AngleMotif's bodies, pins, links and angles with sliders and the claim `expect_sliders` per
slider, as slider_spec.prestep must find it on the initial state: "inactive" (kinv_t <= 0), or "P" followed by the engaged rows of
"L", "M", followed by "-idle" where the slider is solvable along the rail and its limits are not reached.  "P" alone is the slider
that nothing resists along its rail (kinv_n <= 0).

Exact numbers.  A body made at angle 0 has the identity frame bit for bit, so with anchor1 = (0, 0), the world point (0, 0) as anchor2
and the axis (1, 0) the prestep's s is the body's x bit for bit: that is how at_upper, at_lower and one_ulp_inside sit on and beside
their comparisons, and how e_zero has e = (0, 0) exactly.

ON_A_COMPARISON would name the cases that sit exactly on a comparison of the prestep and that the float64 reference, deciding on
float64 positions, takes the other way; such a case would be left out of the comparison of impulses with the reference, by name and
with its reason.  There is none: the cases on a comparison are built from numbers exact in either precision (s = 0.5, limits 0.5, -1,
2, the float above 0.5; kinv_n = 0 from an arm (2, 0) along the axis (1, 0)), so the reference decides them alike."""
import numpy as np

from phyx_amd.api import slider_dtype
from angle_corpus import AngleMotif, DT, G      # noqa: F401 (DT, G: the tests')
from link_corpus import up

F = np.float32
ON_A_COMPARISON = ()


class SliderMotif(AngleMotif):
    def __init__(self, name):
        AngleMotif.__init__(self, name)
        self._sliders, self.expect_sliders = [], []

    def slider(self, a, b, anchor1, anchor2, axis, lower, upper, hertz=0.0, zeta=0.0, speed=0.0, force=0.0, impulse=0.0, axis_impulse=0.0,
               motor_impulse=0.0, expect="PL"):
        self._sliders.append((a, b, anchor1, anchor2, axis, lower, upper, hertz, zeta, speed, force, impulse, axis_impulse, motor_impulse, 0))
        self.expect_sliders.append(expect)
        return len(self._sliders) - 1

    @property
    def sliders(self):
        p = np.zeros(len(self._sliders), dtype=slider_dtype)
        for k, row in enumerate(self._sliders):
            p[k] = row
        return p

    def unit_graph(self):
        """body1, body2 of the units (pins, links, angles, sliders) and the static flags"""
        b1, b2, st = AngleMotif.unit_graph(self)
        s = self.sliders
        return b1 + s["body1"].tolist(), b2 + s["body2"].tolist(), st

    def device_world(self, phyx_amd, gravity=None):
        w = AngleMotif.device_world(self, phyx_amd, gravity)
        got = w.add_sliders(self.sliders)
        assert got.tolist() == list(range(len(self._sliders)))
        return w


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def build(name, tether=False):
    """the case; with `tether` the carriage of every slider also carries a pin to the world (off its centre: a pin at the centre, solved
    last, leaves a linear velocity of exactly 0 in float64 and rounding noise in float32, which no relative metric can compare), a rope
    to the world that never engages and an angle to the world whose limits are never reached: the four kinds then share a component,
    hence a class sequence, and under PHX_PIN_GROUP_PINS=1 the component exceeds the cap and runs through the trailing group's kernels"""
    m = SliderMotif(name)
    CASES[name](m)
    if tether:
        for i in sorted({row[0] for row in m._sliders}):
            x, y = m.rows[i][0], m.rows[i][1]
            static = bool(m.is_static()[i])
            m.pin_at(i, -1, (x + 1.0, y + 0.5))
            fixed = static or (i in m.masses and m.masses[i][0] == 0.0)
            m.link(i, -1, (0.0, 0.0), (x + 3.0, y + 4.0), 0.0, 1.0e6, expect="inactive" if fixed else "idle")
            stiff = static or (i in m.masses and m.masses[i][1] == 0.0)
            m.angle(i, -1, -100.0, 100.0, expect="inactive" if stiff else "idle")
    return m


O = (0.0, 0.0)
X = (1.0, 0.0)
MOVING = (3.0, -2.0, 0.25)


def _one(m, x, lower, upper, vel=MOVING, **kw):
    """one dynamic body at (x, 0), frame the identity, its centre on the world rail through the origin along +x: s == x exactly"""
    a = m.body(x, 0.0, angle=0.0, vel=vel)
    m.slider(a, -1, O, O, X, lower, upper, **kw)
    return a


# -- the geometry --
@case
def e_zero(m):
    """the carriage's anchor exactly on the rail's: e = (0, 0), s = 0, C = 0 on both rows; nothing divides by |e|"""
    _one(m, 0.0, 0.0, 0.0)


@case
def rail_rotated(m):
    """the rail is a dynamic body at 0.6 rad: n is the axis turned with it, and differs from `axis`"""
    b = m.body(0.0, 0.0, angle=0.6, half=(6.0, 1.0), vel=(0.5, 1.0, -0.2))
    a = m.body(40.0, 30.0, angle=0.2, vel=(-2.0, 1.0, 0.3))
    m.slider(a, b, (1.0, 0.5), (2.0, -1.0), X, 45.0, 45.0)


@case
def unnormalised_axis(m):
    """axis (3, 4): len = 5, n = (0.6, 0.8) rounded"""
    a = m.body(10.0, 5.0, angle=0.3, vel=MOVING)
    m.slider(a, -1, (0.5, 0.25), (1.0, 2.0), (3.0, 4.0), 9.0, 9.0)


@case
def short_axis(m):
    """axis of length 2^-9, just above what add accepts: the same n after the division"""
    a = m.body(10.0, 5.0, angle=0.3, vel=MOVING)
    m.slider(a, -1, (0.5, 0.25), (1.0, 2.0), (0.0, 2.0 ** -9), -50.0, 50.0, expect="P-idle")


@case
def world_as_body2(m):
    """two dynamic bodies on a common rail and one of them limited against the world"""
    a = m.body(0.0, 0.0, angle=0.4, vel=(1.0, 0.0, 0.3))
    b = m.body(40.0, 0.0, angle=0.9, vel=(-1.0, 2.0, -0.4))
    m.slider(b, a, (0.5, 0.0), (1.0, 1.0), (1.0, 0.2), 30.0, 30.0)
    m.slider(a, -1, (0.0, 0.5), (0.0, 1.0), (0.0, 1.0), -0.2, 0.2, expect="PL")


@case
def far_along_the_rail(m):
    """the carriage 5000 along a rail that turns: B's arm rb' is long, and the rail's w moves the carriage's point fast"""
    b = m.body(0.0, 0.0, angle=0.0, half=(6.0, 1.0), vel=(0.0, 0.0, 0.01))
    a = m.body(5000.0, 2.0, angle=0.1, vel=(0.0, 50.0, 0.0))
    m.slider(a, b, (0.5, 0.0), (1.0, 0.0), X, 0.0, 6000.0, speed=3.0, force=1.0e6, expect="PM-idle")


# -- the activity rule --
@case
def static_static(m):
    a = m.body(0.0, 0.0, static=True)
    b = m.body(40.0, 0.0, static=True)
    m.slider(a, b, O, O, X, 0.0, 0.0, force=5.0, speed=1.0, expect="inactive")


@case
def no_inverse_mass(m):
    """neither body can translate: both kinv come from the inertias and the arms alone"""
    a = m.body(0.0, 0.0, angle=0.2, mass=(0.0, 0.004), vel=(0.0, 0.0, 0.5))
    b = m.body(40.0, 0.0, angle=0.7, mass=(0.0, 0.002), vel=(0.0, 0.0, -0.3))
    m.slider(a, b, (2.0, 1.0), (-3.0, 2.0), (1.0, 1.0), 20.0, 20.0, force=1.0e6, speed=0.5, expect="PLM")


@case
def p_alone(m):
    """no inverse mass and the arm (2, 0) along the axis (1, 0): ra x n = 0 exactly, kinv_n = 0 with kinv_t = 4 iA > 0: L and M are
    off, their stored impulses become 0, P runs"""
    a = m.body(0.0, 0.0, angle=0.0, mass=(0.0, 0.004), vel=(0.0, 0.0, 0.5))
    m.slider(a, -1, (2.0, 0.0), (2.0, 1.0), X, 0.0, 0.0, force=4.0, speed=1.0, axis_impulse=3.0, motor_impulse=-0.01, expect="P")


@case
def stored_impulses_on_inactive(m):
    """a slider that turns inactive reads its three impulses 0"""
    a = m.body(0.0, 0.0, static=True)
    m.slider(a, -1, O, (0.0, 1.0), X, 0.0, 0.0, force=4.0, impulse=2.0, axis_impulse=3.0, motor_impulse=-0.05, expect="inactive")


# -- the limit decision, on and beside its comparisons (s == the body's x exactly) --
@case
def at_upper(m):
    """s = 0.5 == upper: the upper limit engaged with C = 0"""
    _one(m, 0.5, -1.0, 0.5)


@case
def at_lower(m):
    """s = 0.5 == lower: the lower limit engaged with C = 0"""
    _one(m, 0.5, 0.5, 2.0, vel=(-3.0, -2.0, 0.25))


@case
def one_ulp_inside(m):
    """upper is the float above s: idle, and the stored axis impulse becomes 0"""
    _one(m, 0.5, -1.0, up(0.5), axis_impulse=-2.0, expect="P-idle")


# -- the kinds of row L --
@case
def lock(m):
    a = m.body(3.0, 4.0, angle=0.5, vel=(2.0, 1.0, 0.4))
    m.slider(a, -1, (1.0, -0.5), (0.0, 1.0), (2.0, 1.0), 4.0, 4.0, impulse=0.3, axis_impulse=-0.2)


@case
def spring(m):
    a = m.body(3.0, 4.0, angle=0.5, vel=(2.0, 1.0, 0.4))
    m.slider(a, -1, (1.0, -0.5), (0.0, 1.0), (2.0, 1.0), 1.0, 1.0, hertz=2.0, zeta=0.3, axis_impulse=0.5)


@case
def spring_with_motor(m):
    a = m.body(3.0, 4.0, angle=0.5, vel=(2.0, 1.0, 0.4))
    m.slider(a, -1, (1.0, -0.5), (0.0, 1.0), (2.0, 1.0), 1.0, 1.0, hertz=2.0, zeta=0.3, speed=-1.0, force=4000.0, axis_impulse=0.5, motor_impulse=0.25,
             expect="PLM")


# -- the clamps --
@case
def warm_start_of_the_wrong_sign(m):
    """s = 2 past the upper limit 1 with a stored axis impulse > 0: clamped to 0 at the prestep"""
    _one(m, 2.0, -1.0, 1.0, vel=(0.0, 0.0, 0.0), axis_impulse=2.5)


@case
def motor_saturated_against_limit(m):
    """s = -2 below the lower limit -1, the motor (weak, its stored impulse beyond its range) pushing further down: M saturates at
    -max_force dt, then L holds"""
    _one(m, -2.0, -1.0, 1.0, vel=(0.5, 0.0, 0.0), speed=-50.0, force=3.0e-3, motor_impulse=-50.0, expect="PLM")


@case
def motor_with_idle_limit(m):
    _one(m, 0.25, -1.0, 1.0, speed=2.0, force=1.0e6, axis_impulse=-1.0, expect="PM-idle")


NAMES = tuple(CASES)
assert len(ON_A_COMPARISON) * 6 <= len(NAMES)


def state_of(w):
    """a slider's prestep record as the cases' `expect_sliders` names it"""
    if not w.active:
        return "inactive"
    return "P" + ("L" if w.lrow else "") + ("M" if w.mrow else "") + ("-idle" if w.idle else "")
