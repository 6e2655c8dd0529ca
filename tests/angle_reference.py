"""The angles (include/phyx_amd.h ANGLES) for the pass in float64 (tests/unit_reference.py), written from the mechanics with the means of
tests/pin_reference.py - generalised velocities q = (vx, vy, w), Jacobians, rotation matrices - and not from tests/angle_spec.py.

An angle's constraint is scalar and touches w only: J_a = J_b = (0, 0, 1), so

    kinv = J_a W_a J_a^T + J_b W_b J_b^T,   cdot = J_b q_b - J_a q_a,   push p: q_a -= W_a J_a^T p, q_b += W_b J_b^T p

exactly as a link's row.  The angle itself comes from the bodies' orientations, the counter-clockwise angles of their xVectors
(the header defines theta on the xVectors alone): the engine's w is clockwise-positive (pin_reference.point_jacobian), a body's
orientation falls by w dt per step, and theta, the CLOCKWISE angle of B against A, is orientation(A) - orientation(B) - so that
d theta / dt = cdot, which tests/test_angles_cpu.py checks against the integrator.  phi = theta - mid is brought into [-PI, PI] with the header's constants, so that the two sides hold the same lock.

Rows: L with the header's kinds (lock, soft, limits: one engaged at the prestep or none, the impulse clamped to its sign) and M, the
motor (cdot driven to motor_speed, its impulse clamped to +- max_torque dt), M before L.  Every decision is taken in float64 on
float64 angles: a case that sits exactly on a comparison in float32 may fall the other way here (tests/angle_corpus.py
ON_A_COMPARISON)."""
import numpy as np

import link_reference as lref
import pin_reference as ref

PI = float(np.float32(3.1415927))
TWO_PI = float(np.float32(6.2831855))
J_W = np.array([[0.0, 0.0, 1.0]])


def orientation(st, i):
    """the counter-clockwise angle of body i's xVector (pin_reference.free_state's); the world: 0"""
    return np.arctan2(st.rot[i][1, 0], st.rot[i][0, 0]) if i >= 0 else st.dtype(0)


def relative_angle(st, a, b):
    """the clockwise angle of B's frame against A's, in [-pi, pi]: a clockwise turn lowers a body's orientation, so it is
    orientation(A) - orientation(B), less the full turns"""
    t = orientation(st, a) - orientation(st, b)
    return st.dtype(np.remainder(t + np.pi, 2 * np.pi) - np.pi) if abs(t) > np.pi else t


def _angle(st, angle, dt):
    t = st.dtype
    a, b = int(angle["body1"]), int(angle["body2"])
    j = J_W.astype(t)
    kinv = (j @ np.diag(st.w[a]) @ j.T)[0, 0]
    if b >= 0:
        kinv = kinv + (j @ np.diag(st.w[b]) @ j.T)[0, 0]
    theta = relative_angle(st, a, b)
    lower, upper, hertz, zeta, speed, torque = (t(angle[f]) for f in ("lower", "upper", "hertz", "damping_ratio", "motor_speed", "max_torque"))
    phi = theta - (lower + upper) / 2
    if phi > t(PI):
        phi = phi - t(TWO_PI)
    elif phi < -t(PI):
        phi = phi + t(TWO_PI)
    half = (upper - lower) / 2
    solvable = bool(kinv > 0)
    lo, hi, c, lrow = -np.inf, np.inf, t(0), solvable
    if lower == upper:
        c = phi
    elif phi >= half:
        c, hi = phi - half, 0.0
    elif phi <= -half:
        c, lo = phi + half, 0.0
    else:
        lrow = False
    gamma, bias = t(0), c * t(ref.BETA) / t(dt)
    if hertz > 0 and solvable:
        mass, omega = 1 / kinv, t(TWO_PI) * hertz
        dmp, stiff = 2 * mass * zeta * omega, mass * omega * omega
        gamma = 1 / (t(dt) * (dmp + t(dt) * stiff))
        bias = c * t(dt) * stiff * gamma
    mrow = solvable and bool(torque > 0)
    return a, b, j, kinv, theta, (lrow, gamma, bias, lo, hi), (mrow, speed, torque * t(dt))


deviation = lref.deviation
