"""sleep_spec on the CPU oracle: the rule's decisions are written into OracleWorld's live bodies() view between the steps, which is
what the contract says a sleeping world is (sleep_spec.py).  Shared by test_sleep_cpu.py and by the GPU tests' scene checks."""
import numpy as np

import sleep_spec

DT = 1.0 / 60.0
PARAMS = (0.5, 0.05, 0.5)      # 2.5 x the rest speeds of tilted(12) (test_sleep_cpu.py), and half a second
BOX = (0.0, 260.0, 0.0, 6.0, 6.0)      # the box dropped on the resting pile
BOX_STEP = 330


def apply_to_view(bodies, state, slept, woken):
    """the contract's edits on a live bodies view: a sleeper is static with zero velocities, a woken body has its saved masses"""
    for i in slept:
        bodies["inv_mass"][i] = 0.0; bodies["inv_inertia"][i] = 0.0
        bodies["velocity"]["x"][i] = 0.0; bodies["velocity"]["y"][i] = 0.0; bodies["angular_velocity"][i] = 0.0
    for i in woken:
        bodies["inv_mass"][i] = state["inv_mass"][i]; bodies["inv_inertia"][i] = state["inv_inertia"][i]


def run(oracle, scene, steps, params=PARAMS, box_step=BOX_STEP, box=BOX, gravity=-200.0, dt=DT):
    """-> a list with one record per step: dict(state, bodies (copies, after the rule's edits), slept, woken)"""
    w = oracle.OracleWorld(gravity=gravity)
    w.add_scene(scene)
    p = sleep_spec.Params(*params)
    state = sleep_spec.new_state(len(scene["px"]))
    out = []
    for step in range(steps):
        if step == box_step:
            w.add_body(*box)
            state = sleep_spec.grown(state, len(w.bodies()))
        w.update(dt, oracle.SOLVE_SCALAR, oracle.ISLAND_SINGLE, 15, 15)
        bodies = w.bodies()
        slept, woken = sleep_spec.decide_records(state, bodies, w.manifolds(), None, None, p, dt)
        apply_to_view(bodies, state, slept, woken)
        out.append(dict(state=state.copy(), bodies=bodies.copy(), slept=slept, woken=woken))
    return out
