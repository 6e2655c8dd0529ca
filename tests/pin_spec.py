"""The definition of the pin pass (include/phyx_amd.h PINS): scalar float32, every operation rounded on its own, no fused
multiply-add, IEEE division.  The device kernels (phyx_amd/csrc/pin_kernels.h) follow this file operation for operation.

The pass itself is unit_spec.solve_units, which walks prestep, warm, sweep and store below (and the other kinds') and edits
bodies["velocity"], bodies["angular_velocity"] and pins["impulse"] in place: the prestep and the warm start of every pin in the slot
order `order`, then `iterations` sweeps in slot order.  `bodies` is a rigid_body_dtype array (the oracle World's own, or a copy), `pins`
a pin_dtype array.

The engine's angularVelocity is CLOCKWISE-positive: IntegratePosition rotates the frame by -(angularVelocity * dt) (ref: World.cpp:63)
and the contact limiters project it with n x r, not r x n (ref: Solver.cpp:559-560).  So the velocity of the point r of a body is
v - w x r = (v.x + w r.y, v.y - w r.x), and an impulse P at r changes w by -i (r x P).  Written with the counter-clockwise cross
product (-w r.y, w r.x) the pass pumps energy into everything that turns: a pendulum climbs above its release height and a chain
comes apart within a second.  unit_spec.step_free rotates as the reference does, so the CPU suite sees that.
"""
import numpy as np

F = np.float32
BETA = F(0.2)

# The activity rule: a pin is active where det > DET_FLOOR * (k11 * k22), both sides in float32 as written in prestep.
# K is singular in real arithmetic where nothing resists the impulse along some direction: no inverse mass on either side and
# lever arms that are parallel (or one body that cannot turn, or an anchor at a centre) — a wheel on a fixed axle pinned off-centre
# to the world, two such wheels pinned on the line through their axles.  There det = k11 k22 - k12^2 is exactly 0 and the float32
# expression returns its own rounding error, which `det > 0` took for a determinant (1/det of noise; the body left spinning).
# How large that error is, in units of u = 2^-24 (one rounding) times k11 k22, to first order: with ms = 0 each of k11, k22 is per
# body a term of two rounded products, and one rounded sum of two non-negative terms (which adds 1 u to the larger of their errors):
# 3 u each, their rounded product 7 u.  k12's two terms have the same sign where the arms are parallel, so likewise 3 u, squared 6 u,
# the rounded square 7 u, and k12^2 = k11 k22 there.  The difference rounds relative to its result and cannot change its sign.  So
# the noise is at most 14 u k11 k22 (10 u for the single wheel, whose second body contributes nothing), and 16 u = 2^-20 clears it.
# A well-posed pin is nowhere near: det / (k11 k22) >= 1 / cond(K), and a pin of condition 1e6 has lost every digit float32
# could give its impulse anyway.
DET_FLOOR = F(2.0 ** -20)


class _Pin:
    __slots__ = ("a", "b", "rax", "ray", "rbx", "rby", "k11", "k12", "k22", "inv_det", "biasx", "biasy", "ma", "ia", "mb", "ib",
                 "px", "py", "active", "write_a", "write_b", "c")


def _static(m, i):
    return m == 0 and i == 0


def prestep(bodies, pin, beta, dt=None):
    p = _Pin()
    a, b = int(pin["body1"]), int(pin["body2"])
    p.a, p.b = a, b
    A = bodies[a]
    a1x, a1y = F(pin["anchor1"][0]), F(pin["anchor1"][1])
    a2x, a2y = F(pin["anchor2"][0]), F(pin["anchor2"][1])
    p.ma, p.ia = F(A["inv_mass"]), F(A["inv_inertia"])
    p.rax = F(F(A["xv"]["x"]) * a1x) + F(F(A["yv"]["x"]) * a1y)
    p.ray = F(F(A["xv"]["y"]) * a1x) + F(F(A["yv"]["y"]) * a1y)
    pax, pay = F(A["pos"]["x"]) + p.rax, F(A["pos"]["y"]) + p.ray
    if b >= 0:
        B = bodies[b]
        p.mb, p.ib = F(B["inv_mass"]), F(B["inv_inertia"])
        p.rbx = F(F(B["xv"]["x"]) * a2x) + F(F(B["yv"]["x"]) * a2y)
        p.rby = F(F(B["xv"]["y"]) * a2x) + F(F(B["yv"]["y"]) * a2y)
        pbx, pby = F(B["pos"]["x"]) + p.rbx, F(B["pos"]["y"]) + p.rby
    else:
        p.mb = p.ib = p.rbx = p.rby = F(0)
        pbx, pby = a2x, a2y
    cx, cy = pbx - pax, pby - pay
    p.c = (cx, cy)
    ms = p.ma + p.mb
    p.k11 = (ms + (p.ia * p.ray) * p.ray) + (p.ib * p.rby) * p.rby
    p.k12 = -((p.ia * p.rax) * p.ray) - (p.ib * p.rbx) * p.rby
    p.k22 = (ms + (p.ia * p.rax) * p.rax) + (p.ib * p.rbx) * p.rbx
    det = p.k11 * p.k22 - p.k12 * p.k12
    p.active = bool(det > DET_FLOOR * (p.k11 * p.k22))
    with np.errstate(divide="ignore", invalid="ignore"):
        p.inv_det = F(1) / det
    p.biasx, p.biasy = cx * beta, cy * beta
    p.px = F(pin["impulse"][0]) if p.active else F(0)
    p.py = F(pin["impulse"][1]) if p.active else F(0)
    p.write_a = not _static(p.ma, p.ia)
    p.write_b = b >= 0 and not _static(p.mb, p.ib)
    return p


def _vel(bodies, i):
    if i < 0:
        return F(0), F(0), F(0)
    return F(bodies["velocity"]["x"][i]), F(bodies["velocity"]["y"][i]), F(bodies["angular_velocity"][i])


def _put(bodies, i, v):
    bodies["velocity"]["x"][i], bodies["velocity"]["y"][i], bodies["angular_velocity"][i] = v


def apply(bodies, p, px, py):
    """vA -= mA P, wA += iA (ra x P), vB += mB P, wB -= iB (rb x P); a static body and the world are not written.  The signs of the
    angular terms are the engine's: its angularVelocity is clockwise-positive (module docstring)."""
    if p.write_a:
        vx, vy, w = _vel(bodies, p.a)
        _put(bodies, p.a, (vx - p.ma * px, vy - p.ma * py, w + p.ia * (p.rax * py - p.ray * px)))
    if p.write_b:
        vx, vy, w = _vel(bodies, p.b)
        _put(bodies, p.b, (vx + p.mb * px, vy + p.mb * py, w - p.ib * (p.rbx * py - p.rby * px)))


def sweep(bodies, p):
    vax, vay, wa = _vel(bodies, p.a)
    vbx, vby, wb = _vel(bodies, p.b)
    ubx, uby = vbx + wb * p.rby, vby - wb * p.rbx
    uax, uay = vax + wa * p.ray, vay - wa * p.rax
    rx, ry = -((ubx - uax) + p.biasx), -((uby - uay) + p.biasy)
    dx = p.inv_det * (p.k22 * rx - p.k12 * ry)
    dy = p.inv_det * (p.k11 * ry - p.k12 * rx)
    p.px = p.px + dx
    p.py = p.py + dy
    apply(bodies, p, dx, dy)


def warm(bodies, p):
    apply(bodies, p, p.px, p.py)


def store(pins, k, p):
    pins["impulse"][k] = (p.px, p.py)


def make_bodies(rows):
    """rigid_body_dtype records for rows (px, py, half_x, half_y, static) with AddBody's masses (ref: RigidBody.h:15-36), angle 0."""
    from phyx_amd.api import rigid_body_dtype
    b = np.zeros(len(rows), dtype=rigid_body_dtype)
    for i, (px, py, sx, sy, static) in enumerate(rows):
        b["index"][i] = i
        b["pos"][i] = (px, py)
        b["xv"][i], b["yv"][i] = (1.0, 0.0), (0.0, 1.0)
        b["geom_size"][i] = (sx, sy)
        mass = F(1e-5) * (F(sx) * F(sy))
        inertia = mass * (F(sx) * F(sx) + F(sy) * F(sy))
        if not static:
            b["inv_mass"][i], b["inv_inertia"][i] = F(1) / mass, F(1) / inertia
    return b


def chain(links, spacing=10.0, half=(4.0, 1.5), top=(0.0, 300.0), horizontal=True):
    """A chain of `links` boxes hung from the world point `top`: rows for make_bodies and the pins (pin_dtype).  Horizontal chains
    start level with the anchor and swing down."""
    from phyx_amd.api import pin_dtype
    rows, pins = [], np.zeros(links, dtype=pin_dtype)
    for k in range(links):
        off = spacing * (k + 0.5)
        rows.append((top[0] + off, top[1], half[0], half[1], False) if horizontal else (top[0], top[1] - off, half[1], half[0], False))
    h = spacing / 2.0
    for k in range(links):
        near, far = ((-h, 0.0), (h, 0.0)) if horizontal else ((0.0, h), (0.0, -h))
        if k == 0:
            pins[k] = (0, -1, near, top, (0.0, 0.0))
        else:
            pins[k] = (k, k - 1, near, far, (0.0, 0.0))
    return rows, pins
