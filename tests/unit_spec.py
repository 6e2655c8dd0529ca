"""The pin pass over every kind of unit (include/phyx_amd.h PINS ... SLIDERS), once.  What a kind IS stands in its own module -
pin_spec.py, link_spec.py, angle_spec.py, slider_spec.py: scalar float32, every operation rounded on its own - as four functions of one
signature each:

    prestep(bodies, record, beta, dt) -> the unit's work record for this step (p.active: whether it takes part)
    warm(bodies, p)                      the warm start: the stored impulses applied to the bodies' velocities
    sweep(bodies, p)                     one sweep of the unit's rows
    store(units, k, p)                   the impulses of the work record into record k of the kind's list

KINDS is the table of them in the order of the unit numbering: with `lists` one array per kind, unit u counts through the pins, then
the links, then the angles, then the sliders.  solve_units is the pass the device kernels (phyx_amd/csrc/pin_kernels.h) follow: prestep
and warm start of every unit in the slot order `order`, then `iterations` sweeps in slot order, then the store.  A further kind is one
more entry.

Also here: step_free, a minimal free-body stepper - IntegrateVelocity, the units, IntegratePosition as the reference's World does them,
without contacts - with which the CPU suite checks that the specs hold their mechanisms together.
"""
from bisect import bisect_right
from collections import namedtuple

import numpy as np

from phyx_amd import api
import angle_spec
import link_spec
import pin_spec
import slider_spec
from pin_spec import F, BETA

Kind = namedtuple("Kind", "name plural dtype prestep warm sweep store add get remove count")


def _kind(name, spec):
    plural = name + "s"
    return Kind(name, plural, getattr(api, name + "_dtype"), spec.prestep, spec.warm, spec.sweep, spec.store,
                "add_" + plural, plural, "remove_" + plural, name + "_count")


KINDS = (_kind("pin", pin_spec), _kind("link", link_spec), _kind("angle", angle_spec), _kind("slider", slider_spec))
PIN, LINK, ANGLE, SLIDER = range(len(KINDS))


def full(lists):
    """one array per kind: `lists` and an empty array for every trailing kind it leaves out"""
    lists = list(lists)
    return lists + [np.zeros(0, dtype=kind.dtype) for kind in KINDS[len(lists):]]


def solve_units(bodies, lists, order, dt, iterations=8):
    """The whole pass, in place: the bodies' velocities and every list's impulses.  `lists`: up to len(KINDS) arrays in the table's order,
    missing trailing kinds are empty.  -> per kind the work records of the prestep, in the kind's index order."""
    lists = full(lists)
    ends = np.cumsum([len(units) for units in lists]).tolist()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        beta = BETA / F(dt)
        work = []
        for u in order:
            i = bisect_right(ends, int(u))
            k = int(u) - (ends[i - 1] if i else 0)
            work.append((KINDS[i], i, k, KINDS[i].prestep(bodies, lists[i][k], beta, dt)))
        for kind, _, _, p in work:
            if p.active:
                kind.warm(bodies, p)
        for _ in range(int(iterations)):
            for kind, _, _, p in work:
                if p.active:
                    kind.sweep(bodies, p)
        records = [[None] * len(units) for units in lists]
        for kind, i, k, p in work:
            kind.store(lists[i], k, p)
            records[i][k] = p
    return records


def worst_c(pin_records):
    """the largest |C| of the active pins at the prestep (0.0 without any)"""
    return max([float(np.hypot(float(p.c[0]), float(p.c[1]))) for p in pin_records if p.active], default=0.0)


def integrate_position(bodies, dt):
    """IntegratePosition (ref: World.cpp:57-70) on every body; float32, cos and sin in double rounded to float32"""
    for i in range(len(bodies)):
        b = bodies[i]
        px = F(b["pos"]["x"]) + F(b["velocity"]["x"]) * dt
        py = F(b["pos"]["y"]) + F(b["velocity"]["y"]) * dt
        bodies["pos"]["x"][i], bodies["pos"]["y"][i] = px, py
        ang = -(F(b["angular_velocity"]) * dt)            # ref: World.cpp:63 Rotate(-(... + angularVelocity * dt))
        c, s = F(np.cos(np.float64(ang))), F(np.sin(np.float64(ang)))
        xx, xy = F(b["xv"]["x"]), F(b["xv"]["y"])
        nx, ny = xx * c - xy * s, xx * s + xy * c
        n = F(np.sqrt(np.float64(nx * nx + ny * ny)))
        nx, ny = nx / n, ny / n
        bodies["xv"]["x"][i], bodies["xv"]["y"][i] = nx, ny
        bodies["yv"]["x"][i], bodies["yv"]["y"][i] = -ny, nx


def step_free(bodies, lists, order, dt, gravity, iterations=8, force=None, torque=None):
    """IntegrateVelocity (ref: World.cpp:39-55) on dynamic bodies, the units, IntegratePosition; float32, no contacts.  `force`: per body
    (fx, fy), v += inv_mass force dt; `torque`: per body, w += inv_inertia torque dt - a test's own constant loads.
    -> solve_units' work records."""
    dt = F(dt)
    for i in range(len(bodies)):
        if bodies["inv_mass"][i] != 0:
            bodies["velocity"]["y"][i] = F(bodies["velocity"]["y"][i]) + F(gravity) * dt
            if force is not None:
                bodies["velocity"]["x"][i] = F(bodies["velocity"]["x"][i]) + F(F(bodies["inv_mass"][i]) * F(force[i][0])) * dt
                bodies["velocity"]["y"][i] = F(bodies["velocity"]["y"][i]) + F(F(bodies["inv_mass"][i]) * F(force[i][1])) * dt
        if torque is not None and torque[i] != 0:
            bodies["angular_velocity"][i] = F(bodies["angular_velocity"][i]) + F(F(bodies["inv_inertia"][i]) * F(torque[i])) * dt
    work = solve_units(bodies, lists, order, dt, iterations)
    integrate_position(bodies, dt)
    return work
