"""The definition of the links (include/phyx_amd.h LINKS) and of the pass that solves pins and links together: scalar float32, every
operation rounded on its own, no fused multiply-add, IEEE division, correctly rounded square root (numpy's float32 sqrt is).  The
device kernels (phyx_amd/csrc/pin_kernels.h link_prestep, link_delta) follow this file operation for operation.

A link constrains the distance between two anchors, taken exactly as pin_spec.prestep takes a pin's.  The kind follows from the data:
min_length == max_length is a rod, with hertz > 0 a spring (the Box2D soft constraint); min_length < max_length are limits, of which
at most one is engaged, decided at the prestep (a rope is min_length = 0).  A link between its limits is idle: impulse := 0, nothing
else.  That is deliberately not speculative: a limit engages the step after the length overshoots it and the bias pulls it back, and
until then the bodies move bit for bit as they would without the link.

unit_spec.solve_units(bodies, lists, order, dt, iterations) is the whole pass: the units are the pins followed by the links (unit
u < len(pins) is pin u, otherwise link u - len(pins)); prestep and warm start of every unit in the slot order `order`, then
`iterations` sweeps in slot order.  Pin units go through pin_spec.prestep / apply / sweep unchanged.

The activity rule: a link is active where len > LEN_FLOOR and kinv > 0, both in float32 as written in prestep.
  * LEN_FLOOR = 2^-10.  The axis is n = d / len with d = (posB + rb) - (posA + ra), a difference of world coordinates.  Each
    coordinate carries the rounding of its own sum pos + r: half an ulp of its magnitude.  The playfield's coordinates are of order
    2^13 at the most (the broadphase's cells, the scenes' extents), whose ulp is 2^-10: below that length d is nothing but those
    roundings, and n = d / len would turn them into a unit vector that points anywhere - 1 / len of noise, as pin_spec's DET_FLOOR
    keeps 1 / det of noise out.  A well-posed link is nowhere near: anchors a thousandth of a unit apart are no distance to hold.
    (len == 0, the anchors coincident, has no axis at all and falls under the same rule; so does a rope with min_length = 0 at
    len <= min_length.)
  * kinv = mA + mB + iA (ra x n)^2 + iB (rb x n)^2 is a sum of non-negative terms: kinv <= 0 means that every term is 0, both ends
    static or the world, or (invMass 0, invInertia > 0) an axis through the centre that cannot turn the body.  Nothing resists, so
    nothing is solved.  NaN fails both comparisons and is inactive too.
"""
import numpy as np

import pin_spec
from pin_spec import F

LEN_FLOOR = F(2.0 ** -10)
TWO_PI = F(6.2831855)
INF = F(np.inf)


class _Link:
    __slots__ = ("a", "b", "rax", "ray", "rbx", "rby", "nx", "ny", "gamma", "inv_k", "bias", "lo", "hi", "ma", "ia", "mb", "ib",
                 "lam", "active", "clamps", "write_a", "write_b", "len", "c", "idle")


def clamp(x, lo, hi):
    """comparisons, so that a NaN passes through"""
    return lo if x < lo else (hi if x > hi else x)


def prestep(bodies, link, beta, dt):
    with np.errstate(all="ignore"):
        return _prestep(bodies, link, F(beta), F(dt))


def _prestep(bodies, link, beta, dt):
    p = _Link()
    a, b = int(link["body1"]), int(link["body2"])
    p.a, p.b = a, b
    A = bodies[a]
    a1x, a1y = F(link["anchor1"][0]), F(link["anchor1"][1])
    a2x, a2y = F(link["anchor2"][0]), F(link["anchor2"][1])
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
    p.write_a = not pin_spec._static(p.ma, p.ia)
    p.write_b = b >= 0 and not pin_spec._static(p.mb, p.ib)
    dx, dy = pbx - pax, pby - pay
    ln = np.sqrt(F(dx * dx) + F(dy * dy))
    p.len = ln
    p.nx, p.ny = dx / ln, dy / ln
    cra = F(p.rax * p.ny) - F(p.ray * p.nx)
    crb = F(p.rbx * p.ny) - F(p.rby * p.nx)
    kinv = F(F(p.ma + p.mb) + F(F(p.ia * cra) * cra)) + F(F(p.ib * crb) * crb)
    p.active = bool(ln > LEN_FLOOR) and bool(kinv > 0)
    lo_len, hi_len, hertz, zeta = F(link["min_length"]), F(link["max_length"]), F(link["hertz"]), F(link["damping_ratio"])
    p.clamps = bool(lo_len < hi_len)
    p.lo, p.hi, p.idle = -INF, INF, False
    if not p.clamps:
        c = ln - lo_len
    elif ln >= hi_len:
        c = ln - hi_len
        p.hi = F(0)
    elif ln <= lo_len:
        c = ln - lo_len
        p.lo = F(0)
    else:
        c = F(0)
        p.idle = p.active
        p.active = False
    p.c = c
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
    p.inv_k = F(1) / kinv
    p.lam = clamp(F(link["impulse"]), p.lo, p.hi) if p.active else F(0)
    return p


def apply(bodies, p, lam):
    """P = lam n through the pin's own apply"""
    pin_spec.apply(bodies, p, lam * p.nx, lam * p.ny)


def warm(bodies, p):
    apply(bodies, p, p.lam)


def sweep(bodies, p):
    vax, vay, wa = pin_spec._vel(bodies, p.a)
    vbx, vby, wb = pin_spec._vel(bodies, p.b)
    ubx, uby = vbx + wb * p.rby, vby - wb * p.rbx
    uax, uay = vax + wa * p.ray, vay - wa * p.rax
    cdot = F(p.nx * F(ubx - uax)) + F(p.ny * F(uby - uay))
    d = -(p.inv_k * F(F(cdot + p.bias) + F(p.gamma * p.lam)))
    if p.clamps:
        nxt = clamp(p.lam + d, p.lo, p.hi)
        d = nxt - p.lam
        p.lam = nxt
    else:
        p.lam = p.lam + d
    apply(bodies, p, d)


def store(links, k, p):
    links["impulse"][k] = p.lam


def make_links(rows):
    """link_dtype records for rows (body1, body2, anchor1, anchor2, min_length, max_length[, hertz[, damping_ratio[, impulse]]])"""
    from phyx_amd.api import link_dtype
    p = np.zeros(len(rows), dtype=link_dtype)
    for k, r in enumerate(rows):
        r = tuple(r) + (0.0, 0.0, 0.0)[len(r) - 6:]
        p[k] = (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], 0)
    return p
