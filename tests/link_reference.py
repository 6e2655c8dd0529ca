"""The links (include/phyx_amd.h LINKS) for the pass in float64 (tests/unit_reference.py), written from the mechanics with the means of
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


def deviation(x, x_ref):
    """relative to the largest magnitude in x_ref (pin_reference.deviation on one column)"""
    return ref.deviation(np.asarray(x, dtype=np.float64).reshape(-1, 1), np.asarray(x_ref, dtype=np.float64).reshape(-1, 1))
