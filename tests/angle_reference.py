"""The pass over pins, links and angles (include/phyx_amd.h ANGLES) in float64, written from the mechanics with the means of
tests/pin_reference.py - generalised velocities q = (vx, vy, w), Jacobians, rotation matrices - and not from tests/angle_spec.py.
It extends link_reference.solve to the three kinds.

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


class Result:
    __slots__ = ("q", "pin_impulse", "link_impulse", "link_active", "impulse", "motor_impulse", "lrow", "mrow", "theta")


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


def solve(bodies, pins, links, angles, order, dt, iterations=8, dtype=np.float64):
    """The pass on copies, in slot order over the units (pins, links, angles) -> Result: q (n, 3), pin_impulse (pins, 2),
    link_impulse, link_active (links,), impulse, motor_impulse, lrow, mrow, theta (angles,)."""
    st = ref.State(bodies, dtype)
    npins, npl = len(pins), len(pins) + len(links)
    out = Result()
    out.pin_impulse = np.zeros((npins, 2), dtype=dtype)
    out.link_impulse = np.zeros(len(links), dtype=dtype)
    out.link_active = np.zeros(len(links), dtype=bool)
    out.impulse, out.motor_impulse, out.theta = (np.zeros(len(angles), dtype=dtype) for _ in range(3))
    out.lrow, out.mrow = np.zeros(len(angles), dtype=bool), np.zeros(len(angles), dtype=bool)
    beta = dtype(ref.BETA) / dtype(dt)
    work = []
    for u in order:
        u = int(u)
        if u < npins:
            a, b, ja, jb, kk, c = ref._constraint(st, pins[u])
            if ref.well_posed(kk):
                out.pin_impulse[u] = np.asarray(pins["impulse"][u], dtype=dtype)
                work.append(("pin", u, a, b, ja, jb, kk, beta * c))
        elif u < npl:
            k = u - npins
            a, b, ja, jb, keff, gamma, bias, lo, hi, active = lref._link(st, links[k], dt)
            out.link_active[k] = active
            if active:
                out.link_impulse[k] = min(max(dtype(links["impulse"][k]), lo), hi)
                work.append(("link", k, a, b, ja, jb, keff, (gamma, bias, lo, hi)))
        else:
            k = u - npl
            a, b, j, kinv, theta, (lrow, gamma, bias, lo, hi), (mrow, speed, mmax) = _angle(st, angles[k], dt)
            out.theta[k], out.lrow[k], out.mrow[k] = theta, lrow, mrow
            if mrow:
                out.motor_impulse[k] = min(max(dtype(angles["motor_impulse"][k]), -mmax), mmax)
            if lrow:
                out.impulse[k] = min(max(dtype(angles["impulse"][k]), lo), hi)
            if lrow or mrow:
                work.append(("angle", k, a, b, j, j, kinv, (lrow, gamma, bias, lo, hi, mrow, speed, mmax)))

    def push(a, b, ja, jb, p):
        st.q[a] -= st.w[a] * (ja.T @ p)
        if b >= 0:
            st.q[b] += st.w[b] * (jb.T @ p)

    def rel(a, b, ja, jb):
        v = -(ja @ st.q[a])
        return v + jb @ st.q[b] if b >= 0 else v

    for kind, k, a, b, ja, jb, kk, rest in work:
        if kind == "pin":
            push(a, b, ja, jb, out.pin_impulse[k])
        elif kind == "link":
            push(a, b, ja, jb, out.link_impulse[k:k + 1])
        else:
            if rest[5]:
                push(a, b, ja, jb, out.motor_impulse[k:k + 1])
            if rest[0]:
                push(a, b, ja, jb, out.impulse[k:k + 1])
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for kind, k, a, b, ja, jb, kk, rest in work:
                if kind == "pin":
                    dp = np.linalg.solve(kk, -(rel(a, b, ja, jb) + rest)).astype(dtype)
                    out.pin_impulse[k] += dp
                    push(a, b, ja, jb, dp)
                elif kind == "link":
                    gamma, bias, lo, hi = rest
                    new = out.link_impulse[k] - (rel(a, b, ja, jb)[0] + bias + gamma * out.link_impulse[k]) / kk
                    new = min(max(new, lo), hi)
                    push(a, b, ja, jb, np.array([new - out.link_impulse[k]], dtype=dtype))
                    out.link_impulse[k] = new
                else:
                    lrow, gamma, bias, lo, hi, mrow, speed, mmax = rest
                    if mrow:
                        new = out.motor_impulse[k] - (rel(a, b, ja, jb)[0] - speed) / kk
                        new = min(max(new, -mmax), mmax)
                        push(a, b, ja, jb, np.array([new - out.motor_impulse[k]], dtype=dtype))
                        out.motor_impulse[k] = new
                    if lrow:
                        new = out.impulse[k] - (rel(a, b, ja, jb)[0] + bias + gamma * out.impulse[k]) / (kk + gamma)
                        new = min(max(new, lo), hi)
                        push(a, b, ja, jb, np.array([new - out.impulse[k]], dtype=dtype))
                        out.impulse[k] = new
    out.q = st.q
    return out


deviation = lref.deviation
