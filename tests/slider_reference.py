"""The sliders (include/phyx_amd.h SLIDERS) for the pass in float64 (tests/unit_reference.py), written from the mechanics with the means
of tests/pin_reference.py - generalised velocities q = (vx, vy, w), point Jacobians, rotation matrices - and not from
tests/slider_spec.py.

A slider holds the carriage's anchor point pa = pos_a + R_a anchor1 on the line through pb = pos_b + R_b anchor2 along n = R_b axis /
|axis| (the world: R_b = 1).  With e = pa - pb the coordinate along the rail is s = n . e and the distance off it t . e, t = n turned
a quarter counter-clockwise.  Both are functions of the positions, and their rates follow from the velocity of A's material point at pa
and of B's material point that is at pa NOW (a point rigidly attached to the rail): with the point Jacobians J(r) of pin_reference,

    d(u . e)/dt = u . (J(ra) q_a - J(pa - pos_b) q_b)        for u in {n, t}, u turning with B

(the turning of u contributes (w_b x u) . e, which is what moving B's arm from rb to pa - pos_b = rb + e accounts for).  So each row is
a scalar constraint with the Jacobian rows u^T J(ra), u^T J(pa - pos_b), solved as a link's row:

    kinv = j_a W_a j_a^T + j_b W_b j_b^T,   d_lambda = -(cdot + bias + gamma lambda) / (kinv + gamma)

Rows: P across the rail (hard, always on), L along it with the header's kinds (lock, soft, limits: one engaged at the prestep or none,
the impulse clamped to its sign), M the motor (cdot_n driven to motor_speed, its impulse clamped to +- max_force dt); per sweep M, L, P.
Every decision is taken in float64 on float64 positions: a case that sits exactly on a comparison in float32 may fall the other way
here (tests/slider_corpus.py ON_A_COMPARISON)."""
import numpy as np

import link_reference as lref
import pin_reference as ref

TWO_PI = lref.TWO_PI


def rail(st, slider):
    """-> (a, b, ra, arm_b, e, n, t) in st.dtype: arm_b = pa - pos_b, B's arm to the carriage's anchor point"""
    t_ = st.dtype
    a, b = int(slider["body1"]), int(slider["body2"])
    ra = st.rot[a] @ np.asarray(slider["anchor1"], dtype=t_)
    pa = st.pos[a] + ra
    axis = np.asarray(slider["axis"], dtype=t_)
    if b >= 0:
        pb = st.pos[b] + st.rot[b] @ np.asarray(slider["anchor2"], dtype=t_)
        axis = st.rot[b] @ axis
        arm_b = pa - st.pos[b]
    else:
        pb = np.asarray(slider["anchor2"], dtype=t_)
        arm_b = np.zeros(2, dtype=t_)
    n = axis / np.sqrt(axis @ axis)
    return a, b, ra, arm_b, pa - pb, n, np.array([-n[1], n[0]], dtype=t_)


def translation(st, slider):
    _, _, _, _, e, n, _ = rail(st, slider)
    return n @ e


def _slider(st, slider, dt):
    t_ = st.dtype
    a, b, ra, arm_b, e, n, t = rail(st, slider)
    ja = ref.point_jacobian(ra, t_)
    jb = ref.point_jacobian(arm_b, t_) if b >= 0 else np.zeros((2, 3), dtype=t_)
    wa = np.diag(st.w[a])
    wb = np.diag(st.w[b]) if b >= 0 else np.zeros((3, 3), dtype=t_)

    def row(u):
        # (pin_reference's push / rel take cdot = j_b q_b - j_a q_a: the rows enter negated, so that cdot is A's point against B's)
        ra_, rb_ = -(u @ ja), -(u @ jb)
        return ra_[None, :], rb_[None, :], ra_ @ wa @ ra_ + rb_ @ wb @ rb_

    jta, jtb, kinv_t = row(t)
    jna, jnb, kinv_n = row(n)
    active = bool(kinv_t > 0)
    solvable = active and bool(kinv_n > 0)
    s = n @ e
    lower, upper, hertz, zeta, speed, force = (t_(slider[f]) for f in ("lower", "upper", "hertz", "damping_ratio", "motor_speed", "max_force"))
    lo, hi, c, lrow = -np.inf, np.inf, t_(0), solvable
    if lower == upper:
        c = s - lower
    elif s >= upper:
        c, hi = s - upper, 0.0
    elif s <= lower:
        c, lo = s - lower, 0.0
    else:
        lrow = False
    beta = t_(ref.BETA) / t_(dt)
    gamma, bias = t_(0), c * beta
    if hertz > 0 and solvable:
        mass, omega = 1 / kinv_n, t_(TWO_PI) * hertz
        dmp, stiff = 2 * mass * zeta * omega, mass * omega * omega
        gamma = 1 / (t_(dt) * (dmp + t_(dt) * stiff))
        bias = c * t_(dt) * stiff * gamma
    mrow = solvable and bool(force > 0)
    return a, b, s, active, (jta, jtb, kinv_t, (t @ e) * beta), (lrow, jna, jnb, kinv_n, gamma, bias, lo, hi), (mrow, speed, force * t_(dt))


deviation = lref.deviation
