"""The definition of the angles (include/phyx_amd.h ANGLES) and of the pass that solves pins, links and angles together: scalar
float32, every operation rounded on its own, no fused multiply-add, IEEE division.  The device kernels (phyx_amd/csrc/pin_kernels.h
angle_prestep, angle_warm, angle_sweep) follow this file operation for operation.

An angle constrains the relative angle of two bodies, or of a body against the world (body2 = -1: the identity frame, w = 0).  With
xA, xB the bodies' xVector:

    c = xA . xB,  s = xA.x xB.y - xA.y xB.x,  theta = float32(arctan2(float64(-s), float64(c)))

the double-precision arctan2 rounded to float32 (the rule of the integrators' cos / sin), in the prestep only.  The engine's
angularVelocity is clockwise-positive (pin_spec.py), theta is the clockwise angle of B against A, and d theta / dt = wB - wA: the sign
every row below is written in.  Against the world the world is B, so a body1 turning with w > 0 LOSES w dt of theta per step, and a
free body2 against a resting body1 gains it (tests/test_angles_cpu.py pins both to unit_spec.step_free).

    mid = (lower + upper) * 0.5,  half = (upper - lower) * 0.5,  phi = theta - mid, wrapped once with the float32 constants PI, TWO_PI:
    phi > PI: phi - TWO_PI;  phi < -PI: phi + TWO_PI

so a lock at 3 rad does not jump where theta crosses pi.  |phi| <= PI afterwards, so limits with half > PI - a range wider than
2 PI - are never engaged: that is how a pure motor is written.

kinv = iA + iB.  !(kinv > 0): the unit is INACTIVE, both impulses become 0 and nothing else happens (NaN fails the comparison too).

The row L follows from the data, decided at the prestep and not speculative, as a rope's limit (link_spec.py):
    lower == upper, hertz == 0   a lock:    C = phi, impulse unbounded, bias = C * (0.2 / dt), gamma = 0
    lower == upper, hertz > 0    a spring:  C = phi, the Box2D soft constraint with link_spec's formulas and mass = 1 / kinv
    lower <  upper               limits:    phi >= half: C = phi - half, impulse <= 0;  phi <= -half: C = phi + half, impulse >= 0
                                            (bias as the lock's); otherwise L is idle: impulse := 0
The row M, the motor, is on where max_torque > 0: it drives wB - wA to motor_speed with its accumulated impulse clamped to
+- max_torque * dt.  Off: motor_impulse := 0.  A unit with neither row engaged is inactive.

The warm start applies M's clamped impulse, then L's, each where its row is on.  A sweep is M, then L on the velocities M left
(Box2D's order).  Applying d: wA -= iA d, wB += iB d; linear velocities are not touched; a static body is not written.

unit_spec.solve_units(bodies, lists, order, dt, iterations) is the whole pass over the units: the pins, then the links, then the
angles.  Pin and link units go through pin_spec / link_spec unchanged.
"""
import numpy as np

import pin_spec
from link_spec import clamp
from pin_spec import F

PI = F(3.1415927)
TWO_PI = F(6.2831855)
INF = F(np.inf)


class _Angle:
    __slots__ = ("a", "b", "ia", "ib", "inv_k", "inv_kg", "gamma", "bias", "lo", "hi", "speed", "mmax", "lam", "mlam",
                 "active", "lrow", "mrow", "clamps", "write_a", "write_b", "theta", "phi", "c", "idle")


def theta(bodies, a, b):
    """the relative angle as the prestep takes it"""
    A = bodies[a]
    xax, xay = F(A["xv"]["x"]), F(A["xv"]["y"])
    if b >= 0:
        xbx, xby = F(bodies[b]["xv"]["x"]), F(bodies[b]["xv"]["y"])
    else:
        xbx, xby = F(1), F(0)
    c = F(xax * xbx) + F(xay * xby)
    s = F(xax * xby) - F(xay * xbx)
    return F(np.arctan2(np.float64(-s), np.float64(c)))


def prestep(bodies, angle, beta, dt):
    with np.errstate(all="ignore"):
        return _prestep(bodies, angle, F(beta), F(dt))


def _prestep(bodies, angle, beta, dt):
    p = _Angle()
    a, b = int(angle["body1"]), int(angle["body2"])
    p.a, p.b = a, b
    ma, p.ia = F(bodies[a]["inv_mass"]), F(bodies[a]["inv_inertia"])
    mb, p.ib = (F(bodies[b]["inv_mass"]), F(bodies[b]["inv_inertia"])) if b >= 0 else (F(0), F(0))
    p.write_a = not pin_spec._static(ma, p.ia)
    p.write_b = b >= 0 and not pin_spec._static(mb, p.ib)
    p.theta = theta(bodies, a, b)
    lower, upper, hertz, zeta = F(angle["lower"]), F(angle["upper"]), F(angle["hertz"]), F(angle["damping_ratio"])
    mid, half = F(lower + upper) * F(0.5), F(upper - lower) * F(0.5)
    phi = p.theta - mid
    if phi > PI:
        phi = phi - TWO_PI
    elif phi < -PI:
        phi = phi + TWO_PI
    p.phi = phi
    kinv = p.ia + p.ib
    solvable = bool(kinv > 0)
    p.clamps = bool(lower < upper)
    p.lo, p.hi, lrow = -INF, INF, True
    if not p.clamps:
        c = phi
    elif phi >= half:
        c = phi - half
        p.hi = F(0)
    elif phi <= -half:
        c = phi + half
        p.lo = F(0)
    else:
        c = F(0)
        lrow = False
    p.c = c
    p.inv_k = F(1) / kinv
    if hertz > 0:
        mass = F(1) / kinv
        omega = TWO_PI * hertz
        dmp = F(F(F(2) * mass) * zeta) * omega
        k = F(mass * omega) * omega
        p.gamma = F(1) / F(dt * F(dmp + F(dt * k)))
        p.bias = F(F(c * dt) * k) * p.gamma
        kinv = kinv + p.gamma
    else:
        p.gamma = F(0)
        p.bias = c * beta
    p.inv_kg = F(1) / kinv
    p.speed = F(angle["motor_speed"])
    p.mmax = F(angle["max_torque"]) * dt
    p.mrow = solvable and bool(F(angle["max_torque"]) > 0)
    p.idle = solvable and not lrow                  # the limits are not engaged this step
    p.lrow = solvable and lrow
    p.active = p.lrow or p.mrow
    p.mlam = clamp(F(angle["motor_impulse"]), -p.mmax, p.mmax) if p.mrow else F(0)
    p.lam = clamp(F(angle["impulse"]), p.lo, p.hi) if p.lrow else F(0)
    return p


def _w(bodies, i):
    return F(bodies["angular_velocity"][i]) if i >= 0 else F(0)


def apply(bodies, p, d):
    """wA -= iA d, wB += iB d; a static body and the world are not written"""
    if p.write_a:
        bodies["angular_velocity"][p.a] = _w(bodies, p.a) - F(p.ia * d)
    if p.write_b:
        bodies["angular_velocity"][p.b] = _w(bodies, p.b) + F(p.ib * d)


def warm(bodies, p):
    if p.mrow:
        apply(bodies, p, p.mlam)
    if p.lrow:
        apply(bodies, p, p.lam)


def sweep(bodies, p):
    if p.mrow:
        cdot = _w(bodies, p.b) - _w(bodies, p.a)
        nxt = clamp(p.mlam + -(p.inv_k * F(cdot - p.speed)), -p.mmax, p.mmax)
        d = nxt - p.mlam
        p.mlam = nxt
        apply(bodies, p, d)
    if p.lrow:
        cdot = _w(bodies, p.b) - _w(bodies, p.a)
        d = -(p.inv_kg * F(F(cdot + p.bias) + F(p.gamma * p.lam)))
        if p.clamps:
            nxt = clamp(p.lam + d, p.lo, p.hi)
            d = nxt - p.lam
            p.lam = nxt
        else:
            p.lam = p.lam + d
        apply(bodies, p, d)


def store(angles, k, p):
    angles["impulse"][k], angles["motor_impulse"][k] = p.lam, p.mlam


def make_angles(rows):
    """angle_dtype records for rows (body1, body2, lower, upper[, hertz[, damping_ratio[, motor_speed[, max_torque[, impulse[,
    motor_impulse]]]]]])"""
    from phyx_amd.api import angle_dtype
    p = np.zeros(len(rows), dtype=angle_dtype)
    for k, r in enumerate(rows):
        r = tuple(r) + (0.0,) * (10 - len(r))
        p[k] = r
    return p
