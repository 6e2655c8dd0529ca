"""The definition of the sliders (include/phyx_amd.h SLIDERS) and of the pass that solves pins, links, angles and sliders together:
scalar float32, every operation rounded on its own, no fused multiply-add, IEEE division, correctly rounded sqrt.  The device kernels
(phyx_amd/csrc/pin_kernels.h slider_prestep, slider_warm, slider_sweep) follow this file operation for operation.

A slider holds a point of body1 (the carriage) on a line of body2 (the rail; body2 = -1: the world, whose frame is the identity and
whose velocities are 0).  ra, rb are the rotated anchors, exactly pin_spec's, and

    e = (posA + ra) - (posB + rb)                       against the world: (posA + ra) - anchor2
    a = the axis rotated by B's frame as an anchor is   the world: the axis itself
    len = sqrt(a.x a.x + a.y a.y),  n = a / len,  t = (-n.y, n.x)
    s = n . e  the carriage's coordinate along the rail,  t . e  its distance off the rail

all in the prestep.  Both rows act at the carriage's anchor point on both bodies: A's arm is ra, B's is rb' = rb + e, which carries the
wB term of an axis that turns with the rail: d s / dt = n . de/dt + (wB x n) . e = n . ((vA + wA x ra) - (vB + wB x rb')).
With the engine's clockwise-positive angularVelocity (pin_spec.py), w x r = (w r.y, -w r.x), and r x u = r.x u.y - r.y u.x, for u in {t, n}:

    cdot_u = u . ((vA + wA x ra) - (vB + wB x rb'))
    kinv_u = ((mA + mB) + (iA (ra x u)) (ra x u)) + (iB (rb' x u)) (rb' x u)
    apply lam along u, P = lam u:  vA += mA P,  wA -= iA (ra x P),  vB -= mB P,  wB += iB (rb' x P)

A carriage that moves along +n gains s (tests/test_sliders_cpu.py pins that to step_free).  A static body is not written.

!(kinv_t > 0): the slider is INACTIVE this step, its three impulses become 0 and nothing else happens.  !(kinv_n > 0) with kinv_t > 0:
rows L and M are off, their impulses become 0, and P runs.  Nothing divides by |e|: e = 0 is an ordinary case.

The rows:
    P   perpendicular: C = t . e, impulse unbounded, bias = C * (0.2 / dt); on whenever the slider is active
    L   along the axis on s, angle_spec's row L word for word:
        lower == upper, hertz == 0   a lock:    C = s - lower, impulse unbounded, bias = C * (0.2 / dt), gamma = 0
        lower == upper, hertz > 0    a spring:  C = s - lower, link_spec's soft constraint with mass = 1 / kinv_n
        lower <  upper               limits:    s >= upper: C = s - upper, impulse <= 0;  s <= lower: C = s - lower, impulse >= 0
                                                (bias as the lock's); otherwise L is idle: axis_impulse := 0
        decided at the prestep and not speculative, as a rope's limit
    M   the motor, on where max_force > 0: it drives cdot_n to motor_speed with its accumulated impulse clamped to +- max_force * dt.
        Off: motor_impulse := 0.

The warm start applies M's clamped impulse, then L's, then P's, each where its row is on.  A sweep is M, then L, then P, each on the
velocities the row before left: the hard row has the last word.

unit_spec.solve_units(bodies, lists, order, dt, iterations) is the whole pass over the units: the pins, then the links,
then the angles, then the sliders.  The first three go through pin_spec / link_spec / angle_spec unchanged.
"""
import numpy as np

import pin_spec
from link_spec import clamp, TWO_PI
from pin_spec import F

INF = F(np.inf)
AXIS_FLOOR = F(2.0 ** -20)      # add's rule: axis.x^2 + axis.y^2 > 2^-20


class _Slider:
    __slots__ = ("a", "b", "rax", "ray", "rbx", "rby", "nx", "ny", "ma", "ia", "mb", "ib", "inv_kt", "inv_kn", "inv_kng", "gamma",
                 "bias_t", "bias", "lo", "hi", "speed", "mmax", "plam", "lam", "mlam", "active", "lrow", "mrow", "clamps",
                 "write_a", "write_b", "ex", "ey", "s", "ct", "c", "idle", "kinv_t", "kinv_n")


def geometry(bodies, slider):
    """(ra, rb, e, n) as the prestep takes them"""
    a, b = int(slider["body1"]), int(slider["body2"])
    A = bodies[a]
    a1x, a1y = F(slider["anchor1"][0]), F(slider["anchor1"][1])
    a2x, a2y = F(slider["anchor2"][0]), F(slider["anchor2"][1])
    ax, ay = F(slider["axis"][0]), F(slider["axis"][1])
    rax = F(F(A["xv"]["x"]) * a1x) + F(F(A["yv"]["x"]) * a1y)
    ray = F(F(A["xv"]["y"]) * a1x) + F(F(A["yv"]["y"]) * a1y)
    pax, pay = F(A["pos"]["x"]) + rax, F(A["pos"]["y"]) + ray
    if b >= 0:
        B = bodies[b]
        rbx = F(F(B["xv"]["x"]) * a2x) + F(F(B["yv"]["x"]) * a2y)
        rby = F(F(B["xv"]["y"]) * a2x) + F(F(B["yv"]["y"]) * a2y)
        pbx, pby = F(B["pos"]["x"]) + rbx, F(B["pos"]["y"]) + rby
        wx = F(F(B["xv"]["x"]) * ax) + F(F(B["yv"]["x"]) * ay)
        wy = F(F(B["xv"]["y"]) * ax) + F(F(B["yv"]["y"]) * ay)
    else:
        rbx = rby = F(0)
        pbx, pby = a2x, a2y
        wx, wy = ax, ay
    ex, ey = pax - pbx, pay - pby
    ln = np.sqrt(F(wx * wx) + F(wy * wy))
    return (rax, ray), (rbx, rby), (ex, ey), (wx / ln, wy / ln)


def translation(bodies, slider):
    """s = n . e as the prestep takes it"""
    with np.errstate(all="ignore"):
        _, _, (ex, ey), (nx, ny) = geometry(bodies, slider)
        return F(nx * ex) + F(ny * ey)


def prestep(bodies, slider, beta, dt):
    with np.errstate(all="ignore"):
        return _prestep(bodies, slider, F(beta), F(dt))


def _prestep(bodies, slider, beta, dt):
    p = _Slider()
    a, b = int(slider["body1"]), int(slider["body2"])
    p.a, p.b = a, b
    p.ma, p.ia = F(bodies[a]["inv_mass"]), F(bodies[a]["inv_inertia"])
    p.mb, p.ib = (F(bodies[b]["inv_mass"]), F(bodies[b]["inv_inertia"])) if b >= 0 else (F(0), F(0))
    p.write_a = not pin_spec._static(p.ma, p.ia)
    p.write_b = b >= 0 and not pin_spec._static(p.mb, p.ib)
    (p.rax, p.ray), (rbx, rby), (ex, ey), (p.nx, p.ny) = geometry(bodies, slider)
    p.ex, p.ey = ex, ey
    p.rbx, p.rby = rbx + ex, rby + ey                      # rb'
    s = F(p.nx * ex) + F(p.ny * ey)
    ct = F(p.nx * ey) - F(p.ny * ex)                       # t . e, t = (-n.y, n.x)
    p.s, p.ct = s, ct
    # r x t = r.x n.x + r.y n.y;  r x n = r.x n.y - r.y n.x
    cat = F(p.rax * p.nx) + F(p.ray * p.ny)
    cbt = F(p.rbx * p.nx) + F(p.rby * p.ny)
    can = F(p.rax * p.ny) - F(p.ray * p.nx)
    cbn = F(p.rbx * p.ny) - F(p.rby * p.nx)
    ms = p.ma + p.mb
    kinv_t = F(ms + F(F(p.ia * cat) * cat)) + F(F(p.ib * cbt) * cbt)
    kinv_n = F(ms + F(F(p.ia * can) * can)) + F(F(p.ib * cbn) * cbn)
    p.kinv_t, p.kinv_n = kinv_t, kinv_n
    p.active = bool(kinv_t > 0)
    solvable = p.active and bool(kinv_n > 0)
    p.inv_kt = F(1) / kinv_t
    p.bias_t = ct * beta
    lower, upper, hertz, zeta = F(slider["lower"]), F(slider["upper"]), F(slider["hertz"]), F(slider["damping_ratio"])
    p.clamps = bool(lower < upper)
    p.lo, p.hi, lrow = -INF, INF, True
    if not p.clamps:
        c = s - lower
    elif s >= upper:
        c = s - upper
        p.hi = F(0)
    elif s <= lower:
        c = s - lower
        p.lo = F(0)
    else:
        c = F(0)
        lrow = False
    p.c = c
    kinv = kinv_n
    p.inv_kn = F(1) / kinv
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
    p.inv_kng = F(1) / kinv
    p.speed = F(slider["motor_speed"])
    p.mmax = F(slider["max_force"]) * dt
    p.mrow = solvable and bool(F(slider["max_force"]) > 0)
    p.idle = solvable and not lrow                  # the limits are not engaged this step
    p.lrow = solvable and lrow
    p.mlam = clamp(F(slider["motor_impulse"]), -p.mmax, p.mmax) if p.mrow else F(0)
    p.lam = clamp(F(slider["axis_impulse"]), p.lo, p.hi) if p.lrow else F(0)
    p.plam = F(slider["impulse"]) if p.active else F(0)
    return p


def apply(bodies, p, px, py):
    """P = (px, py) at the carriage's anchor point: vA += mA P, wA -= iA (ra x P), vB -= mB P, wB += iB (rb' x P)"""
    if p.write_a:
        vx, vy, w = pin_spec._vel(bodies, p.a)
        pin_spec._put(bodies, p.a, (vx + p.ma * px, vy + p.ma * py, w - p.ia * (p.rax * py - p.ray * px)))
    if p.write_b:
        vx, vy, w = pin_spec._vel(bodies, p.b)
        pin_spec._put(bodies, p.b, (vx - p.mb * px, vy - p.mb * py, w + p.ib * (p.rbx * py - p.rby * px)))


def _rel(bodies, p):
    """(vA + wA x ra) - (vB + wB x rb')"""
    vax, vay, wa = pin_spec._vel(bodies, p.a)
    vbx, vby, wb = pin_spec._vel(bodies, p.b)
    uax, uay = vax + wa * p.ray, vay - wa * p.rax
    ubx, uby = vbx + wb * p.rby, vby - wb * p.rbx
    return uax - ubx, uay - uby


def warm(bodies, p):
    if p.mrow:
        apply(bodies, p, p.mlam * p.nx, p.mlam * p.ny)
    if p.lrow:
        apply(bodies, p, p.lam * p.nx, p.lam * p.ny)
    apply(bodies, p, p.plam * -p.ny, p.plam * p.nx)


def sweep(bodies, p):
    if p.mrow:
        rx, ry = _rel(bodies, p)
        cdot = F(p.nx * rx) + F(p.ny * ry)
        nxt = clamp(p.mlam + -(p.inv_kn * F(cdot - p.speed)), -p.mmax, p.mmax)
        d = nxt - p.mlam
        p.mlam = nxt
        apply(bodies, p, d * p.nx, d * p.ny)
    if p.lrow:
        rx, ry = _rel(bodies, p)
        cdot = F(p.nx * rx) + F(p.ny * ry)
        d = -(p.inv_kng * F(F(cdot + p.bias) + F(p.gamma * p.lam)))
        if p.clamps:
            nxt = clamp(p.lam + d, p.lo, p.hi)
            d = nxt - p.lam
            p.lam = nxt
        else:
            p.lam = p.lam + d
        apply(bodies, p, d * p.nx, d * p.ny)
    rx, ry = _rel(bodies, p)
    cdot = F(p.nx * ry) - F(p.ny * rx)
    d = -(p.inv_kt * F(cdot + p.bias_t))
    p.plam = p.plam + d
    apply(bodies, p, d * -p.ny, d * p.nx)


def store(sliders, k, p):
    sliders["impulse"][k], sliders["axis_impulse"][k], sliders["motor_impulse"][k] = p.plam, p.lam, p.mlam


def make_sliders(rows):
    """slider_dtype records for rows (body1, body2, anchor1, anchor2, axis, lower, upper[, hertz[, damping_ratio[, motor_speed[,
    max_force[, impulse[, axis_impulse[, motor_impulse]]]]]]])"""
    from phyx_amd.api import slider_dtype
    p = np.zeros(len(rows), dtype=slider_dtype)
    for k, r in enumerate(rows):
        r = tuple(r) + (0.0,) * (14 - len(r))
        p[k] = r + (0,)
    return p
