"""Directed angles: single-step worlds of one or two bodies, each named for what it reaches in tests/angle_spec.py (the wrap, the
signed zeros of exactly opposite frames, the limit decision on and beside its comparisons, the activity rule, the clamps, both rows
together).  tests/test_angles_cpu.py proves the claims on the CPU and holds the spec to the float64 reference
(tests/angle_reference.py); tests/test_angle_corpus_gpu.py runs every case on the device, byte for byte against the spec.

A case is an AngleMotif: link_corpus.LinkMotif's bodies, pins and links with angles and the claim `expect_angles` per angle, as
angle_spec.prestep must find it on the initial state: "L", "M" or "LM" (the engaged rows), "idle" (solvable, no row engaged) or
"inactive" (kinv <= 0).

Exact frames.  A body made at angle 0 has the frame (1, 0) bit for bit, so against the world theta = atan2(-0, 1) = -0 and
phi = -mid exactly; `frames` sets a body's xVector to given bits through set_poses / the oracle's set_pose, which is how (-1, +0) and
(-1, -0) - the two exactly opposite frames, s = -0 and s = +0 - are made: no angle's cos / sin gives them.

ON_A_COMPARISON would name the cases that sit exactly on a comparison of the prestep and that the float64 reference, deciding on
float64 angles, takes the other way; such a case would be left out of the comparison of impulses with the reference, by name and
with its reason.  There is none: at_upper, at_lower and one_ulp_inside are built from numbers exact in either precision (theta = -0,
limits -1, 0, 1, 2^-24), so the reference decides them alike; the exactly opposite frames give theta = +-pi, where float32 PI > pi
makes the spec subtract and wrap other numbers than the reference does, and the reference's own float32 run shows the same
deviation (ratios 1.22 and 0.98).  No case is left out of anything."""
import numpy as np

from phyx_amd.api import angle_dtype
from link_corpus import LinkMotif, DT, G      # noqa: F401 (DT, G: the tests')

F = np.float32
ON_A_COMPARISON = ()


class AngleMotif(LinkMotif):
    def __init__(self, name):
        LinkMotif.__init__(self, name)
        self._angles, self.expect_angles, self.frames = [], [], {}
        self.steps = 2

    def angle(self, a, b, lower, upper, hertz=0.0, zeta=0.0, speed=0.0, torque=0.0, impulse=0.0, motor_impulse=0.0, expect="L"):
        self._angles.append((a, b, lower, upper, hertz, zeta, speed, torque, impulse, motor_impulse))
        self.expect_angles.append(expect)
        return len(self._angles) - 1

    @property
    def angles(self):
        p = np.zeros(len(self._angles), dtype=angle_dtype)
        for k, row in enumerate(self._angles):
            p[k] = row
        return p

    def unit_graph(self):
        """body1, body2 of the units (pins, links, angles) and the static flags"""
        b1, b2, st = LinkMotif.unit_graph(self)
        a = self.angles
        return b1 + a["body1"].tolist(), b2 + a["body2"].tolist(), st

    def _pose(self, i):
        x, y = self.frames[i]
        return np.array([self.rows[i][0], self.rows[i][1], x, y, -y, x], dtype=np.float32)

    def oracle_world(self, binding, gravity=None):
        from helpers import oracle_set_pose
        w = LinkMotif.oracle_world(self, binding, gravity)
        for i in self.frames:
            oracle_set_pose(binding, w, i, self._pose(i))
        return w

    def device_world(self, phyx_amd, gravity=None):
        w = LinkMotif.device_world(self, phyx_amd, gravity)
        if self.frames:
            idx = sorted(self.frames)
            w.set_poses(np.asarray(idx, dtype=np.int32), np.stack([self._pose(i) for i in idx]))
        got = w.add_angles(self.angles)
        assert got.tolist() == list(range(len(self._angles)))
        return w


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def build(name, tether=False):
    """the case; with `tether` the first body of every angle also carries a pin to the world at its centre and a rope to the world
    that never engages: pin, link and angle then share a component, hence a class sequence, and under PHX_PIN_GROUP_PINS=1 the
    component exceeds the cap and runs through the trailing group's kernels"""
    m = AngleMotif(name)
    CASES[name](m)
    if tether:
        for i in sorted({row[0] for row in m._angles}):
            x, y = m.rows[i][0], m.rows[i][1]
            m.pin_at(i, -1, (x, y))
            fixed = m.is_static()[i] or (i in m.masses and m.masses[i][0] == 0.0)
            m.link(i, -1, (0.0, 0.0), (x + 3.0, y + 4.0), 0.0, 1.0e6, expect="inactive" if fixed else "idle")
    return m


SPIN = (0.0, 0.0, 0.7)


def _one(m, angle, lower, upper, vel=SPIN, **kw):
    """one dynamic body at the origin at `angle` (theta against the world = angle), an angle unit to the world"""
    a = m.body(0.0, 0.0, angle=angle, vel=vel)
    m.angle(a, -1, lower, upper, **kw)
    return a


# -- the wrap --
@case
def wrap_below_pi(m):
    """theta = 3.1, a lock at 3: phi = 0.1, no wrap"""
    _one(m, 3.1, 3.0, 3.0)


@case
def wrap_above_pi(m):
    """theta = -3.1 (the same frame turned 0.083 further), the lock at 3: phi = -6.1, wrapped to 0.183 - not a jump of a full turn"""
    _one(m, -3.1, 3.0, 3.0)


@case
def opposite_s_minus_zero(m):
    """the frame (-1, +0): s = -0, theta = atan2(+0, -1) = +pi"""
    a = _one(m, 0.0, 3.0, 3.0)
    m.frames[a] = (-1.0, 0.0)


@case
def opposite_s_plus_zero(m):
    """the frame (-1, -0): s = +0, theta = atan2(-0, -1) = -pi, wrapped"""
    a = _one(m, 0.0, 3.0, 3.0)
    m.frames[a] = (-1.0, -0.0)


# -- the limit decision, on and beside its comparisons (theta = -0: phi = -mid exactly) --
@case
def at_upper(m):
    """limits [-1, 0]: phi = 0.5 == half, the upper limit engaged with C = 0"""
    _one(m, 0.0, -1.0, 0.0, vel=(0.0, 0.0, -0.7))


@case
def at_lower(m):
    """limits [0, 1]: phi = -0.5 == -half, the lower limit engaged with C = 0"""
    _one(m, 0.0, 0.0, 1.0)


@case
def one_ulp_inside(m):
    """limits [-1, 2^-24]: mid = -(0.5 - 2^-25), half = 0.5 (1 + 2^-24 rounds to 1): phi is the float below half"""
    _one(m, 0.0, -1.0, 2.0 ** -24, impulse=-2.0, expect="idle")


# -- the activity rule --
@case
def static_static(m):
    a = m.body(0.0, 0.0, static=True)
    b = m.body(40.0, 0.0, static=True)
    m.angle(a, b, 0.0, 0.0, torque=5.0, speed=1.0, expect="inactive")


@case
def no_inertia_one_side(m):
    """body1 cannot turn (invInertia 0, invMass > 0): kinv is body2's alone; body1 is written and its w does not change"""
    a = m.body(0.0, 0.0, mass=(0.02, 0.0), vel=(1.0, 0.0, 0.0))
    b = m.body(40.0, 0.0, vel=(0.0, 1.0, 0.5))
    m.angle(a, b, 0.0, 0.0)


@case
def no_inertia_both(m):
    a = m.body(0.0, 0.0, mass=(0.02, 0.0), vel=(1.0, 0.0, 0.0))
    b = m.body(40.0, 0.0, mass=(0.03, 0.0), vel=(0.0, 1.0, 0.0))
    m.angle(a, b, 0.0, 0.0, torque=3.0, speed=2.0, expect="inactive")


@case
def world_as_body2(m):
    """two dynamic bodies locked to each other and one of them limited against the world"""
    a = m.body(0.0, 0.0, angle=0.4, vel=(0.0, 0.0, 0.3))
    b = m.body(40.0, 0.0, angle=0.9, vel=(0.0, 0.0, -0.4))
    m.angle(b, a, -0.5, -0.5)
    m.angle(a, -1, -0.2, 0.2)


@case
def stored_impulse_on_inactive(m):
    """a unit that turns inactive reads both impulses 0"""
    a = m.body(0.0, 0.0, static=True)
    m.angle(a, -1, 0.0, 0.0, torque=4.0, impulse=3.0, motor_impulse=-0.05, expect="inactive")


# -- the clamps --
@case
def warm_start_of_the_wrong_sign(m):
    """theta = 0.5 past the upper limit 0.3 with a stored impulse > 0: clamped to 0 at the prestep"""
    _one(m, 0.5, -0.3, 0.3, vel=(0.0, 0.0, 0.0), impulse=2.5)


# -- both rows --
@case
def motor_saturated_against_limit(m):
    """theta = -0.5 below the lower limit, the motor (weak, its stored impulse beyond its range) pushing further down: M saturates at
    -max_torque dt, then L holds"""
    _one(m, -0.5, -0.3, 0.3, vel=(0.0, 0.0, 0.2), speed=-5.0, torque=0.03, motor_impulse=-50.0, expect="LM")


@case
def motor_with_idle_limit(m):
    _one(m, 0.1, -0.3, 0.3, speed=2.0, torque=1.0e6, impulse=-1.0, expect="M")


@case
def spring_with_motor(m):
    _one(m, 0.6, 0.2, 0.2, hertz=2.0, zeta=0.3, speed=-1.0, torque=400.0, impulse=0.5, motor_impulse=0.25, expect="LM")


NAMES = tuple(CASES)
assert len(ON_A_COMPARISON) * 6 <= len(NAMES)


def rows_of(w):
    """an angle's prestep record as the cases' `expect_angles` names it: its engaged rows, or idle / inactive"""
    return ("L" if w.lrow else "") + ("M" if w.mrow else "") or ("idle" if w.idle else "inactive")
