"""Shared helpers for the parity tests: scene states produced with the oracle world."""
import ctypes as C

import numpy as np

from oracle import binding as ob
from phyx_amd import scenes


def oracle_world(scene, gravity=-200.0):
    w = ob.OracleWorld(gravity)
    w.add_scene(scene)
    return w


def presolve_state(scene, warm_steps, iters=15, gravity=-200.0):
    """Run `warm_steps` full oracle steps, then everything of the next step that precedes SolveJoints.
    Returns copies of (bodies, contact_points, joints) = the solver's inputs (warm-start impulses included)."""
    w = oracle_world(scene, gravity)
    for _ in range(warm_steps):
        w.update(contact_iters=iters, penetration_iters=iters)
    w.pre_solve()
    return w.bodies().copy(), w.contact_points().copy(), w.joints().copy()


def oracle_set_velocity(ow, i, v):
    b = ow.bodies()
    b["velocity"]["x"][i], b["velocity"]["y"][i], b["angular_velocity"][i] = v[0], v[1], v[2]


def oracle_set_pose(oracle, ow, i, p):
    """coords = ..., then UpdateGeom: the geom copy and the oracle's own RecomputeAABB (ref: RigidBody.h:38-42, Geom.h:79-85)."""
    b = ow.bodies()
    b["pos"]["x"][i], b["pos"]["y"][i], b["xv"]["x"][i], b["xv"]["y"][i], b["yv"]["x"][i], b["yv"]["y"][i] = p
    b["geom_pos"][i], b["geom_xv"][i], b["geom_yv"][i] = b["pos"][i], b["xv"][i], b["yv"][i]
    oracle.lib().phxo_recompute_aabb(C.c_void_p(b.ctypes.data + i * b.dtype.itemsize))


def is_static(bodies):
    return ((bodies["inv_mass"] == 0) & (bodies["inv_inertia"] == 0)).astype(np.uint8)


SMALL_SCENES = {
    "stack2x10": (lambda: scenes.stack(2, 10), 2),
    "stack10x100": (lambda: scenes.stack(10, 100), 3),
    "tilted60": (lambda: scenes.tilted(60), 25),
    "falling600": (lambda: scenes.falling(600, width=90.0, ymax=300.0), 45),
}
