"""The pass over pins, links, angles and sliders (include/phyx_amd.h SLIDERS) in float64, written from the mechanics with the means
of tests/pin_reference.py - generalised velocities q = (vx, vy, w), point Jacobians, rotation matrices - and not from
tests/slider_spec.py.  It extends angle_reference.solve to the four kinds.

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

import angle_reference as aref
import link_reference as lref
import pin_reference as ref

TWO_PI = lref.TWO_PI


class Result:
    __slots__ = ("q", "pin_impulse", "link_impulse", "link_active", "angle_impulse", "angle_motor_impulse", "angle_lrow", "angle_mrow",
                 "impulse", "axis_impulse", "motor_impulse", "active", "lrow", "mrow", "s")


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


def solve(bodies, pins, links, angles, sliders, order, dt, iterations=8, dtype=np.float64):
    """The pass on copies, in slot order over the units (pins, links, angles, sliders) -> Result: q (n, 3), pin_impulse (pins, 2),
    link_impulse, link_active (links,), angle_impulse, angle_motor_impulse, angle_lrow, angle_mrow (angles,), impulse, axis_impulse,
    motor_impulse, active, lrow, mrow, s (sliders,)."""
    st = ref.State(bodies, dtype)
    npins, npl = len(pins), len(pins) + len(links)
    npla = npl + len(angles)
    out = Result()
    out.pin_impulse = np.zeros((npins, 2), dtype=dtype)
    out.link_impulse = np.zeros(len(links), dtype=dtype)
    out.link_active = np.zeros(len(links), dtype=bool)
    out.angle_impulse, out.angle_motor_impulse = np.zeros(len(angles), dtype=dtype), np.zeros(len(angles), dtype=dtype)
    out.angle_lrow, out.angle_mrow = np.zeros(len(angles), dtype=bool), np.zeros(len(angles), dtype=bool)
    out.impulse, out.axis_impulse, out.motor_impulse, out.s = (np.zeros(len(sliders), dtype=dtype) for _ in range(4))
    out.active, out.lrow, out.mrow = (np.zeros(len(sliders), dtype=bool) for _ in range(3))
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
        elif u < npla:
            k = u - npl
            a, b, j, kinv, theta, (lrow, gamma, bias, lo, hi), (mrow, speed, mmax) = aref._angle(st, angles[k], dt)
            out.angle_lrow[k], out.angle_mrow[k] = lrow, mrow
            if mrow:
                out.angle_motor_impulse[k] = min(max(dtype(angles["motor_impulse"][k]), -mmax), mmax)
            if lrow:
                out.angle_impulse[k] = min(max(dtype(angles["impulse"][k]), lo), hi)
            if lrow or mrow:
                work.append(("angle", k, a, b, j, j, kinv, (lrow, gamma, bias, lo, hi, mrow, speed, mmax)))
        else:
            k = u - npla
            a, b, s, active, prow, lrow, mrow = _slider(st, sliders[k], dt)
            out.s[k], out.active[k], out.lrow[k], out.mrow[k] = s, active, lrow[0], mrow[0]
            if not active:
                continue
            if mrow[0]:
                out.motor_impulse[k] = min(max(dtype(sliders["motor_impulse"][k]), -mrow[2]), mrow[2])
            if lrow[0]:
                out.axis_impulse[k] = min(max(dtype(sliders["axis_impulse"][k]), lrow[6]), lrow[7])
            out.impulse[k] = dtype(sliders["impulse"][k])
            work.append(("slider", k, a, b, None, None, None, (prow, lrow, mrow)))

    def push(a, b, ja, jb, p):
        st.q[a] -= st.w[a] * (ja.T @ p)
        if b >= 0:
            st.q[b] += st.w[b] * (jb.T @ p)

    def rel(a, b, ja, jb):
        v = -(ja @ st.q[a])
        return v + jb @ st.q[b] if b >= 0 else v

    def scalar_row(acc, k, a, b, ja, jb, keff, gamma, bias, lo, hi):
        new = acc[k] - (rel(a, b, ja, jb)[0] + bias + gamma * acc[k]) / keff
        new = min(max(new, lo), hi)
        push(a, b, ja, jb, np.array([new - acc[k]], dtype=dtype))
        acc[k] = new

    for kind, k, a, b, ja, jb, kk, rest in work:
        if kind == "pin":
            push(a, b, ja, jb, out.pin_impulse[k])
        elif kind == "link":
            push(a, b, ja, jb, out.link_impulse[k:k + 1])
        elif kind == "angle":
            if rest[5]:
                push(a, b, ja, jb, out.angle_motor_impulse[k:k + 1])
            if rest[0]:
                push(a, b, ja, jb, out.angle_impulse[k:k + 1])
        else:
            prow, lrow, mrow = rest
            if mrow[0]:
                push(a, b, lrow[1], lrow[2], out.motor_impulse[k:k + 1])
            if lrow[0]:
                push(a, b, lrow[1], lrow[2], out.axis_impulse[k:k + 1])
            push(a, b, prow[0], prow[1], out.impulse[k:k + 1])
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for kind, k, a, b, ja, jb, kk, rest in work:
                if kind == "pin":
                    dp = np.linalg.solve(kk, -(rel(a, b, ja, jb) + rest)).astype(dtype)
                    out.pin_impulse[k] += dp
                    push(a, b, ja, jb, dp)
                elif kind == "link":
                    gamma, bias, lo, hi = rest
                    scalar_row(out.link_impulse, k, a, b, ja, jb, kk, gamma, bias, lo, hi)
                elif kind == "angle":
                    lrow, gamma, bias, lo, hi, mrow, speed, mmax = rest
                    if mrow:
                        scalar_row(out.angle_motor_impulse, k, a, b, ja, jb, kk, 0, -speed, -mmax, mmax)
                    if lrow:
                        scalar_row(out.angle_impulse, k, a, b, ja, jb, kk + gamma, gamma, bias, lo, hi)
                else:
                    (jta, jtb, kinv_t, bias_t), (lrow, jna, jnb, kinv_n, gamma, bias, lo, hi), (mrow, speed, mmax) = rest
                    if mrow:
                        scalar_row(out.motor_impulse, k, a, b, jna, jnb, kinv_n, 0, -speed, -mmax, mmax)
                    if lrow:
                        scalar_row(out.axis_impulse, k, a, b, jna, jnb, kinv_n + gamma, gamma, bias, lo, hi)
                    scalar_row(out.impulse, k, a, b, jta, jtb, kinv_t, 0, bias_t, -np.inf, np.inf)
    out.q = st.q
    return out


deviation = lref.deviation
