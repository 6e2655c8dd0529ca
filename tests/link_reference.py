"""The pass over pins and links (include/phyx_amd.h LINKS) in float64, written from the mechanics with the means of
tests/pin_reference.py - generalised velocities, point Jacobians, matrix products - and not from tests/link_spec.py.

A link's constraint is scalar: with the pin's separation d = (pos_b + rb) - (pos_a + ra), len = |d| and n = d / len, its Jacobians
are the rows n^T J(ra), n^T J(rb) of the pin's, and

    kinv = n^T (J_a W_a J_a^T + J_b W_b J_b^T) n
    d_lambda = -(cdot + bias + gamma lambda) / (kinv + gamma),   cdot = n^T (J_b q_b - J_a q_a)

with the header's kinds: rigid (gamma = 0, bias = 0.2 C / dt), soft (Box2D's: gamma = 1 / (dt (dmp + dt k)), bias = C dt k gamma),
limits (one engaged at the prestep or none, the accumulated impulse clamped to its sign).  The kind decisions and the activity rule
are taken in float64 on float64 lengths: a case that sits exactly on one of their comparisons in float32 may fall the other way here
(tests/link_corpus.py ON_A_COMPARISON)."""
import numpy as np

import pin_reference as ref

LEN_FLOOR = 2.0 ** -10
TWO_PI = float(np.float32(6.2831855))          # the header's constant, so that the two sides solve the same spring


class Result:
    __slots__ = ("q", "pin_impulse", "impulse", "active")


def _link(st, link, dt):
    dt_ = st.dtype
    as_pin = {"body1": link["body1"], "body2": link["body2"], "anchor1": link["anchor1"], "anchor2": link["anchor2"]}
    a, b, ja, jb, k, d = ref._constraint(st, as_pin)
    ln = np.sqrt(d @ d)
    with np.errstate(all="ignore"):
        n = d / ln
        kinv = n @ k @ n
    active = bool(ln > LEN_FLOOR) and bool(kinv > 0)
    lo_len, hi_len, hertz, zeta = (dt_(link[f]) for f in ("min_length", "max_length", "hertz", "damping_ratio"))
    lo, hi, c = -np.inf, np.inf, dt_(0)
    if lo_len == hi_len:
        c = ln - lo_len
    elif ln >= hi_len:
        c, hi = ln - hi_len, 0.0
    elif ln <= lo_len:
        c, lo = ln - lo_len, 0.0
    else:
        active = False
    gamma, bias = dt_(0), c * dt_(ref.BETA) / dt_(dt)
    if hertz > 0 and active:
        mass, omega = 1 / kinv, dt_(TWO_PI) * hertz
        dmp, stiff = 2 * mass * zeta * omega, mass * omega * omega
        gamma = 1 / (dt_(dt) * (dmp + dt_(dt) * stiff))
        bias = c * dt_(dt) * stiff * gamma
    return a, b, (n @ ja)[None, :], (n @ jb)[None, :], kinv + gamma, gamma, bias, lo, hi, active


def solve(bodies, pins, links, order, dt, iterations=8, dtype=np.float64):
    """The pass on copies, in slot order over the units (the pins, then the links) -> Result: q (n, 3), pin_impulse (pins, 2),
    impulse (links,), active (links,)."""
    st = ref.State(bodies, dtype)
    npins = len(pins)
    out = Result()
    out.pin_impulse = np.zeros((npins, 2), dtype=dtype)
    out.impulse = np.zeros(len(links), dtype=dtype)
    out.active = np.zeros(len(links), dtype=bool)
    beta = dtype(ref.BETA) / dtype(dt)
    work = []
    for u in order:
        u = int(u)
        if u < npins:
            a, b, ja, jb, kk, c = ref._constraint(st, pins[u])
            if ref.well_posed(kk):
                out.pin_impulse[u] = np.asarray(pins["impulse"][u], dtype=dtype)
                work.append(("pin", u, a, b, ja, jb, kk, beta * c))
        else:
            k = u - npins
            a, b, ja, jb, keff, gamma, bias, lo, hi, active = _link(st, links[k], dt)
            out.active[k] = active
            if active:
                out.impulse[k] = min(max(dtype(links["impulse"][k]), lo), hi)
                work.append(("link", k, a, b, ja, jb, keff, (gamma, bias, lo, hi)))

    def push(a, b, ja, jb, p):
        st.q[a] -= st.w[a] * (ja.T @ p)
        if b >= 0:
            st.q[b] += st.w[b] * (jb.T @ p)

    def rel(a, b, ja, jb):
        v = -(ja @ st.q[a])
        return v + jb @ st.q[b] if b >= 0 else v

    for kind, k, a, b, ja, jb, kk, rest in work:
        push(a, b, ja, jb, out.pin_impulse[k] if kind == "pin" else out.impulse[k:k + 1])
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for kind, k, a, b, ja, jb, kk, rest in work:
                if kind == "pin":
                    dp = np.linalg.solve(kk, -(rel(a, b, ja, jb) + rest)).astype(dtype)
                    out.pin_impulse[k] += dp
                    push(a, b, ja, jb, dp)
                else:
                    gamma, bias, lo, hi = rest
                    new = out.impulse[k] - (rel(a, b, ja, jb)[0] + bias + gamma * out.impulse[k]) / kk
                    new = min(max(new, lo), hi)
                    push(a, b, ja, jb, np.array([new - out.impulse[k]], dtype=dtype))
                    out.impulse[k] = new
    out.q = st.q
    return out


def deviation(x, x_ref):
    """relative to the largest magnitude in x_ref (pin_reference.deviation on one column)"""
    return ref.deviation(np.asarray(x, dtype=np.float64).reshape(-1, 1), np.asarray(x_ref, dtype=np.float64).reshape(-1, 1))
