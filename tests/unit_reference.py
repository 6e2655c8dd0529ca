"""The pin pass over every kind of unit (include/phyx_amd.h PINS ... SLIDERS) in float64: the suite's judge, written from the mechanics
and not from the specs.  What a kind's constraint is stands with the kind - pin_reference._constraint, link_reference._link,
angle_reference._angle, slider_reference._slider, with the metrics the tests judge by - in generalised velocities q = (vx, vy, w),
Jacobians and matrix products.  Here each unit becomes its rows, in the order they are solved in:

    (acc, k, j_a, j_b, keff, gamma, bias, lo, hi)        acc[k]: the row's accumulated impulse in the Result

a scalar row  d_lambda = -(cdot + bias + gamma lambda) / keff,  lambda clamped to [lo, hi],  cdot = j_b q_b - j_a q_a, or - gamma None -
a pin's 2 x 2 block  dP = solve(K, -(cdot + beta C)).  solve() runs the pass as the header defines it: every unit's rows from the poses
in slot order, the warm start of every row, then `iterations` sweeps in slot order.  A static body has W = 0 and is left alone by the
algebra itself.

`dtype` is the precision of every array and of the linear solve: run at float32 the same algorithm measures its own rounding noise.
Whether a pin is well posed is decided in float64 whatever `dtype` is (pin_reference.py)."""
from bisect import bisect_right

import numpy as np

import angle_reference as aref
import link_reference as lref
import pin_reference as pref
import slider_reference as sref
from unit_spec import full


class Result:
    """q (n, 3) the velocities after the pass, and <kind>_<field> per kind in the kind's index order: the impulses, what the prestep
    decided (active, lrow, mrow) and saw (pin_c (pins, 2) the separations, angle_theta, slider_s)"""
    FLOATS = dict(pin=("impulse", "c"), link=("impulse",), angle=("impulse", "motor_impulse", "theta"),
                  slider=("impulse", "axis_impulse", "motor_impulse", "s"))
    FLAGS = dict(pin=("active",), link=("active",), angle=("lrow", "mrow"), slider=("active", "lrow", "mrow"))

    def __init__(self, lists, dtype):
        for (kind, floats), units in zip(self.FLOATS.items(), lists):
            for f in floats:
                setattr(self, kind + "_" + f, np.zeros((len(units), 2) if kind == "pin" else len(units), dtype=dtype))
            for f in self.FLAGS[kind]:
                setattr(self, kind + "_" + f, np.zeros(len(units), dtype=bool))


def _clamped(x, lo, hi):
    return min(max(x, lo), hi)


def _pin_rows(out, st, exact, pins, k, dt):
    a, b, ja, jb, kk, c = pref._constraint(st, pins[k])
    out.pin_c[k] = c
    out.pin_active[k] = pref.well_posed(pref._constraint(exact, pins[k])[4])
    if not out.pin_active[k]:
        return a, b, []
    out.pin_impulse[k] = np.asarray(pins["impulse"][k], dtype=st.dtype)
    return a, b, [(out.pin_impulse, k, ja, jb, kk, None, st.dtype(pref.BETA) / st.dtype(dt) * c, None, None)]


def _link_rows(out, st, exact, links, k, dt):
    a, b, ja, jb, keff, gamma, bias, lo, hi, out.link_active[k] = lref._link(st, links[k], dt)
    if not out.link_active[k]:
        return a, b, []
    out.link_impulse[k] = _clamped(st.dtype(links["impulse"][k]), lo, hi)
    return a, b, [(out.link_impulse, k, ja, jb, keff, gamma, bias, lo, hi)]


def _angle_rows(out, st, exact, angles, k, dt):
    a, b, j, kinv, theta, (lrow, gamma, bias, lo, hi), (mrow, speed, mmax) = aref._angle(st, angles[k], dt)
    out.angle_theta[k], out.angle_lrow[k], out.angle_mrow[k] = theta, lrow, mrow
    rows = []
    if mrow:
        out.angle_motor_impulse[k] = _clamped(st.dtype(angles["motor_impulse"][k]), -mmax, mmax)
        rows.append((out.angle_motor_impulse, k, j, j, kinv, 0, -speed, -mmax, mmax))
    if lrow:
        out.angle_impulse[k] = _clamped(st.dtype(angles["impulse"][k]), lo, hi)
        rows.append((out.angle_impulse, k, j, j, kinv + gamma, gamma, bias, lo, hi))
    return a, b, rows


def _slider_rows(out, st, exact, sliders, k, dt):
    a, b, s, active, (jta, jtb, kinv_t, bias_t), (lrow, jna, jnb, kinv_n, gamma, bias, lo, hi), (mrow, speed, mmax) = sref._slider(st, sliders[k], dt)
    out.slider_s[k], out.slider_active[k], out.slider_lrow[k], out.slider_mrow[k] = s, active, lrow, mrow
    if not active:
        return a, b, []
    rows = []
    if mrow:
        out.slider_motor_impulse[k] = _clamped(st.dtype(sliders["motor_impulse"][k]), -mmax, mmax)
        rows.append((out.slider_motor_impulse, k, jna, jnb, kinv_n, 0, -speed, -mmax, mmax))
    if lrow:
        out.slider_axis_impulse[k] = _clamped(st.dtype(sliders["axis_impulse"][k]), lo, hi)
        rows.append((out.slider_axis_impulse, k, jna, jnb, kinv_n + gamma, gamma, bias, lo, hi))
    out.slider_impulse[k] = st.dtype(sliders["impulse"][k])
    return a, b, rows + [(out.slider_impulse, k, jta, jtb, kinv_t, 0, bias_t, -np.inf, np.inf)]


ROWS = (_pin_rows, _link_rows, _angle_rows, _slider_rows)       # in the order of unit_spec.KINDS


def solve(bodies, lists, order, dt, iterations=8, dtype=np.float64):
    """The pass on copies, in slot order over the units of `lists` (one array per kind, trailing kinds may be left out) -> Result.
    Nothing is edited in place."""
    lists = full(lists)
    st = pref.State(bodies, dtype)
    exact = st if dtype == np.float64 else pref.State(bodies, np.float64)
    out = Result(lists, dtype)
    ends = np.cumsum([len(units) for units in lists]).tolist()
    work = []
    for u in order:
        i = bisect_right(ends, int(u))
        a, b, rows = ROWS[i](out, st, exact, lists[i], int(u) - (ends[i - 1] if i else 0), dt)
        work += [(a, b) + row for row in rows]

    def push(a, b, ja, jb, p):
        st.q[a] -= st.w[a] * (ja.T @ p)
        if b >= 0:
            st.q[b] += st.w[b] * (jb.T @ p)

    def rel(a, b, ja, jb):
        v = -(ja @ st.q[a])
        return v + jb @ st.q[b] if b >= 0 else v

    for a, b, acc, k, ja, jb, keff, gamma, bias, lo, hi in work:
        push(a, b, ja, jb, np.atleast_1d(acc[k]))
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for a, b, acc, k, ja, jb, keff, gamma, bias, lo, hi in work:
                if gamma is None:
                    dp = np.linalg.solve(keff, -(rel(a, b, ja, jb) + bias)).astype(dtype)
                    acc[k] += dp
                else:
                    new = _clamped(acc[k] - (rel(a, b, ja, jb)[0] + bias + gamma * acc[k]) / keff, lo, hi)
                    dp = np.array([new - acc[k]], dtype=dtype)
                    acc[k] = new
                push(a, b, ja, jb, dp)
    out.q = st.q
    return out
