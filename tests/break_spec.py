"""The definition of breakable units (include/phyx_amd.h BREAKS), in the style of pin_spec.py ... slider_spec.py: scalar float32, every
operation rounded on its own, a correctly rounded sqrt.

Every unit of the pin pass has a break limit L, a float32 with 0 < L <= +inf (a new unit's is +inf: unbreakable).  After the pass of a
step with time step dt the impulses the pass stored in the unit's record give its reaction impulse R:

    pin     sqrt(impulse.x impulse.x + impulse.y impulse.y)
    link    fabs(impulse)
    angle   fabs(impulse + motor_impulse)
    slider  a = axis_impulse + motor_impulse;  sqrt(impulse impulse + a a)      (the rows' directions t and n are orthonormal)

The unit breaks in that step iff R > L dt: one float32 product, a strict comparison that is false for a NaN.  An inactive or idle unit
has stored 0 and never breaks.  A broken unit has acted in the step it broke in; before the next step's pass it is gone from its list as
phx_world_remove_<kind> would take it: the others keep their order.  Every break is one event, a step's events ordered by (kind, index).

The choices.  R is taken from the accumulated impulses of the whole step, not from a sweep's: it is what the joint transmitted.  An
angle's and a slider's motor counts: a weld that a motor tears apart has sheared.  The limit is a force (a torque), so that a change
of the time step does not change what a joint carries.  The test is behind the pass and in front of the contacts: what the contacts
add to a joint's load shows in the next step's pass, when the joint resists it.
"""
import numpy as np

import slider_spec
from pin_spec import F

INF = F(np.inf)
PIN, LINK, ANGLE, SLIDER = 0, 1, 2, 3
KINDS = ("pin", "link", "angle", "slider")


def event_dtype():
    from phyx_amd.api import break_event_dtype
    return break_event_dtype


def no_limits(pins, links, angles, sliders):
    """the limits of new units: +inf each, one float32 array per kind"""
    return [np.full(len(l), INF, dtype=np.float32) for l in (pins, links, angles, sliders)]


def reactions(pins, links, angles, sliders):
    """R of every unit from the impulses in its record: one float32 array per kind"""
    with np.errstate(over="ignore", invalid="ignore"):
        rp = np.zeros(len(pins), dtype=np.float32)
        for k in range(len(pins)):
            x, y = F(pins["impulse"][k][0]), F(pins["impulse"][k][1])
            rp[k] = np.sqrt(F(F(x * x) + F(y * y)))
        rl = np.zeros(len(links), dtype=np.float32)
        for k in range(len(links)):
            rl[k] = np.abs(F(links["impulse"][k]))
        ra = np.zeros(len(angles), dtype=np.float32)
        for k in range(len(angles)):
            ra[k] = np.abs(F(F(angles["impulse"][k]) + F(angles["motor_impulse"][k])))
        rs = np.zeros(len(sliders), dtype=np.float32)
        for k in range(len(sliders)):
            p = F(sliders["impulse"][k])
            a = F(F(sliders["axis_impulse"][k]) + F(sliders["motor_impulse"][k]))
            rs[k] = np.sqrt(F(F(p * p) + F(a * a)))
    return [rp, rl, ra, rs]


def breaks(pins, links, angles, sliders, limits, dt, step=0):
    """The events of the step whose pass left the lists as they are, in (kind, index) order: a break_event_dtype array."""
    events = []
    with np.errstate(over="ignore", invalid="ignore"):
        for kind, (units, r, lim) in enumerate(zip((pins, links, angles, sliders), reactions(pins, links, angles, sliders), limits)):
            assert len(lim) == len(units)
            for k in range(len(units)):
                threshold = F(F(lim[k]) * F(dt))
                if r[k] > threshold:
                    events.append((kind, k, int(units["body1"][k]), int(units["body2"][k]), step, r[k], threshold, 0))
    return np.array(events, dtype=event_dtype()) if events else np.zeros(0, dtype=event_dtype())


def settle(pins, links, angles, sliders, limits, events):
    """The lists and the limits without the units the events name: ([pins, links, angles, sliders], limits)."""
    lists, kept = [], []
    for kind, (units, lim) in enumerate(zip((pins, links, angles, sliders), limits)):
        gone = [int(e["index"]) for e in events if int(e["kind"]) == kind]
        lists.append(np.delete(units, gone))
        kept.append(np.delete(np.asarray(lim, dtype=np.float32), gone))
    return lists, kept


def step_free(bodies, pins, links, angles, sliders, limits, order, dt, gravity, iterations=8, force=None, step=0):
    """slider_spec.step_free, then the break test of that pass: -> (events, [the lists as the next step finds them], their limits).
    `order`: the pass's order of units (None: pins, links, angles, sliders, each in index order)."""
    if order is None:
        order = range(len(pins) + len(links) + len(angles) + len(sliders))
    slider_spec.step_free(bodies, pins, links, angles, sliders, order, dt, gravity, iterations, force)
    events = breaks(pins, links, angles, sliders, limits, dt, step)
    lists, kept = settle(pins, links, angles, sliders, limits, events)
    return events, lists, kept
