"""The harness of the units' device tests (tests/test_pins_gpu.py ... test_breaks_gpu.py, test_units_gpu.py): the device World and the
oracle World in lockstep, the spec's pass (tests/unit_spec.py) applied to the oracle's bodies between its pre_solve and its solve on the
device's own schedule of units, every byte of the state and of every kind's list compared after every step; the life cycle by twins; and
the means of the refusal tests.  `lists` is one array per kind in the order of unit_spec.KINDS, the spec's own; everything here walks
that table, so that a further kind is an entry there."""
import ctypes as C

import numpy as np

import phyx_amd
from phyx_amd import Configuration
from phyx_amd.api import pin_dtype
from helpers import oracle_world
from spawn_lockstep import compare
from unit_spec import KINDS
import unit_spec

DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
O, X, Y = (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)


def empty(kind):
    return np.zeros(0, dtype=kind.dtype)


def lists(**units):
    """lists(angles=a, pins=p): one array per kind, by the kinds' plurals; an empty one for every kind not given"""
    assert set(units) <= {kind.plural for kind in KINDS}, units.keys()
    return [units.get(kind.plural, empty(kind)) for kind in KINDS]


def cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def scene(rows):
    """rows (px, py, half_x, half_y, static[, angle]) -> a scenes.py dict"""
    r = np.asarray([row[:4] for row in rows], dtype=np.float32).reshape(-1, 4)
    return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": np.asarray([row[5] if len(row) > 5 else 0.0 for row in rows], dtype=np.float32),
            "sx": r[:, 2].copy(), "sy": r[:, 3].copy(), "static": np.asarray([bool(row[4]) for row in rows], dtype=bool)}


def pins(rows):
    """pin_dtype records for rows (body1, body2, anchor1, anchor2)"""
    p = np.zeros(len(rows), dtype=pin_dtype)
    for k, (a, b, a1, a2) in enumerate(rows):
        p[k] = (a, b, a1, a2, (0.0, 0.0))
    return p


def add(pw, lists):
    """every kind's units to the device world, which numbers them from 0 on"""
    for kind, units in zip(KINDS, lists):
        assert getattr(pw, kind.add)(units).tolist() == list(range(len(units)))


def worlds(scene, lists, gravity=G, with_oracle=True):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    add(pw, lists)
    return pw, (oracle_world(scene, gravity) if with_oracle else None)


def step(oracle, pw, ow, cfg, lists, dt=DT):
    """spawn_lockstep.step with the units: 1. pw.Update  2. ow.pre_solve  3. unit_spec.solve_units on ow.bodies() on the device's own
    schedule of units  4. the oracle's solver on the device's contact schedule  5. ow.integrate_position.
    -> (the schedule, per kind the units' prestep records)"""
    sched = pw.pin_schedule()
    assert sorted(sched["order"].tolist()) == list(range(sum(len(units) for units in lists)))
    pw.Update(dt, cfg)
    ow.pre_solve(dt)
    work = unit_spec.solve_units(ow.bodies(), lists, sched["order"], dt, pw.pin_iterations)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(dt)
    return sched, work


def lists_of(pw):
    return [getattr(pw, kind.get)() for kind in KINDS]


def check(pw, ow, lists, s):
    compare(pw, ow, s)
    for kind, got, units in zip(KINDS, lists_of(pw), lists):
        assert got.tobytes() == units.tobytes(), "%s differ at step %d" % (kind.plural, s)


def counts(pw):
    return [getattr(pw, kind.count)() for kind in KINDS]


# ---- the life cycle, by twins ----
def same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)
    for kind, x, y in zip(KINDS, lists_of(a), lists_of(b)):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (kind.plural, what)


def twin(state, lists):
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*state)
    for kind, units in zip(KINDS, lists):
        getattr(pb, kind.add)(units)
    return pb


def run_twins(pa, pb, steps, what):
    c = cfg()
    for s in range(steps):
        pa.Update(DT, c)
        pb.Update(DT, c)
        same(pa, pb, "at step %d after %s" % (s, what))


def remapped(units, new):
    """the units that phx_world_remove_bodies keeps, their bodies renumbered by `new` (removal_spec.new_index)"""
    keep = np.array([new[p["body1"]] >= 0 and (p["body2"] < 0 or new[p["body2"]] >= 0) for p in units], dtype=bool)
    kept = units[keep].copy()
    kept["body1"] = new[kept["body1"]]
    kept["body2"] = np.where(kept["body2"] < 0, -1, new[np.maximum(kept["body2"], 0)])
    return kept


# ---- the refusals ----
def snapshot_of(pw):
    return (pw.bodies.tobytes(),) + tuple(units.tobytes() for units in lists_of(pw)) + (pw.pin_schedule_builds(),)


def unchanged(pw, before):
    assert snapshot_of(pw) == before


def message(pw):
    return pw.L.phx_last_error().decode()


def raw_add(pw, kind, recs, count=None, null=False):
    """phx_world_add_<kind>s itself: -> its status"""
    p = np.ascontiguousarray(recs, dtype=kind.dtype)
    call = getattr(pw.L, "phx_world_" + kind.add)
    return call(pw.h, None if null else p.ctypes.data_as(C.c_void_p), len(p) if count is None else count, None)
