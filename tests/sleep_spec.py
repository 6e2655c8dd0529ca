"""The definition of sleeping (include/phyx_amd.h SLEEPING), in the style of break_spec.py: scalar float32, every operation rounded on
its own.

The contract.  A world that sleeps is, byte for byte, a world that does not sleep on which somebody applies edits between every two
steps: for every body the rule puts to sleep set_inverse_masses(body, 0, 0) and set_velocities(body, 0, 0, 0), for every body it wakes
set_inverse_masses(body, saved values).  A sleeper is a static body to every kernel of the step; this file only decides who sleeps and
who wakes.

State per body: asleep, timer (float32), saved {inv_mass, inv_inertia}.  A body is DYNAMIC iff inv_mass != 0 or inv_inertia != 0,
MOBILE iff dynamic or asleep, AWAKE iff dynamic and not asleep.

The pass runs once per step on the state the step leaves behind (after IntegratePosition), in this order:

  1. timers: an awake body with vx vx + vy vy <= lin lin and w w <= ang ang has timer += dt, every other awake body timer = 0
     (products and sums rounded separately);
  2. edges: every manifold with point_count > 0 whose two bodies are mobile and neither is a sensor; every unit of every kind whose
     two bodies are mobile (a unit to the world, body2 == -1, is no edge);
  3. components of that graph, labelled by their smallest body index;
  4. a sleeper is STRUCK if it shares a point_count > 0 manifold with a non-mobile body that has a nonzero velocity or angular
     velocity word (a conveyor, a kinematic platform);
  5. per component: if it holds a sleeper and also an awake body or a struck sleeper, every sleeper in it wakes (masses restored) and
     timer = 0 for the whole component; if it holds no sleeper and its minimum timer is >= time_to_sleep, all of it sleeps (masses
     saved, then zeroed; velocity and angular velocity +0); anything else stays as it is.

In the step in which something lands on a sleeper the sleeper still acts as a static; it wakes at that step's end.
The units are the lists as the step's pin pass solved them: a unit that broke in this step (break_spec.py) is still an edge in it.
"""
import numpy as np

F = np.float32
BODY_SENSOR = 1

state_dtype = np.dtype([("asleep", "<i4"), ("timer", "<f4"), ("inv_mass", "<f4"), ("inv_inertia", "<f4")])      # phx_sleep_state


class Params:
    def __init__(self, linear_tolerance, angular_tolerance, time_to_sleep):
        self.lin, self.ang, self.time_to_sleep = F(linear_tolerance), F(angular_tolerance), F(time_to_sleep)


def new_state(n):
    """the column of n new bodies: awake, timer 0, nothing saved"""
    return np.zeros(n, dtype=state_dtype)


def grown(state, n):
    """the column after a spawn up to n bodies"""
    return np.concatenate([state, new_state(n - len(state))])


def shown(state, inv_mass, inv_inertia):
    """what phx_world_get_sleep_states shows: the body's own masses whether asleep or not"""
    out = state.copy()
    awake = out["asleep"] == 0
    out["inv_mass"][awake] = np.asarray(inv_mass, dtype=np.float32)[awake]
    out["inv_inertia"][awake] = np.asarray(inv_inertia, dtype=np.float32)[awake]
    return out


def _find(parent, i):
    while parent[i] != i:
        i = parent[i]
    return i


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)      # the root is the smallest body


def labels(mobile, pairs):
    """label[i] = the smallest body of i's component over the edges `pairs` (both ends mobile), -1 for a body that is not mobile"""
    n = len(mobile)
    parent = list(range(n))
    for a, b in pairs:
        if 0 <= a < n and 0 <= b < n and mobile[a] and mobile[b]:
            _union(parent, int(a), int(b))
    return np.array([_find(parent, i) if mobile[i] else -1 for i in range(n)], dtype=np.int64)


def unit_pairs(lists):
    """(body1, body2) of every unit of every kind (arrays with body1, body2 fields; None: an empty list)"""
    out = []
    for units in lists or ():
        if units is not None:
            out += [(int(a), int(b)) for a, b in zip(units["body1"], units["body2"])]
    return out


def decide(state, inv_mass, inv_inertia, vx, vy, w, manifolds, units, flags, params, dt):
    """One pass.  `state` is updated in place (timers, asleep, saved masses); the body arrays are the step's result and are not touched.
    manifolds: body1, body2, point_count fields; units: (body1, body2) pairs; flags: per-body PHX_BODY_* words or None.
    -> (slept, woken): ascending body indices.  The caller applies the contract's edits for them."""
    n = len(state)
    inv_mass = np.asarray(inv_mass, dtype=np.float32); inv_inertia = np.asarray(inv_inertia, dtype=np.float32)
    vx = np.asarray(vx, dtype=np.float32); vy = np.asarray(vy, dtype=np.float32); w = np.asarray(w, dtype=np.float32)
    asleep = state["asleep"] != 0
    dynamic = (inv_mass != 0) | (inv_inertia != 0)
    mobile = dynamic | asleep
    awake = dynamic & ~asleep
    lin2, ang2, dt = F(params.lin * params.lin), F(params.ang * params.ang), F(dt)
    # 1. timers
    for i in range(n):
        if not awake[i]:
            continue
        calm = F(F(vx[i] * vx[i]) + F(vy[i] * vy[i])) <= lin2 and F(w[i] * w[i]) <= ang2
        state["timer"][i] = F(state["timer"][i] + dt) if calm else F(0)
    # 2. - 4. edges, components, struck sleepers
    sensor = np.zeros(n, dtype=bool) if flags is None else (np.asarray(flags, dtype=np.uint32) & BODY_SENSOR) != 0
    pairs, struck = [], np.zeros(n, dtype=bool)
    moving = (vx.view(np.uint32) != 0) | (vy.view(np.uint32) != 0) | (w.view(np.uint32) != 0)      # any nonzero word: -0.0 moves
    for m in manifolds:
        a, b = int(m["body1"]), int(m["body2"])
        if int(m["point_count"]) <= 0:
            continue
        if mobile[a] and mobile[b] and not sensor[a] and not sensor[b]:
            pairs.append((a, b))
        for s, o in ((a, b), (b, a)):
            if asleep[s] and not mobile[o] and moving[o]:
                struck[s] = True
    pairs += [(a, b) for a, b in units if b >= 0]
    label = labels(mobile, pairs)
    # 5. per component
    slept, woken = [], []
    for root in np.unique(label[label >= 0]):
        members = np.flatnonzero(label == root)
        has_sleeper = asleep[members].any()
        if has_sleeper and (awake[members].any() or struck[members].any()):
            for i in members:
                if asleep[i]:
                    state["asleep"][i] = 0
                    woken.append(int(i))
                state["timer"][i] = F(0)
        elif not has_sleeper and state["timer"][members].min() >= params.time_to_sleep:
            for i in members:
                state["asleep"][i] = 1
                state["inv_mass"][i] = inv_mass[i]; state["inv_inertia"][i] = inv_inertia[i]
                slept.append(int(i))
    return sorted(slept), sorted(woken)


def decide_records(state, bodies, manifolds, lists, flags, params, dt):
    """decide() on 128-byte body records (the World's or the oracle's bodies()) and the unit lists"""
    return decide(state, bodies["inv_mass"], bodies["inv_inertia"], bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"],
                  manifolds, unit_pairs(lists), flags, params, dt)


def wake_components(state, bodies_named, manifolds, units, flags=None):
    """phx_world_wake_bodies: the sleeping component of each named body wakes -> woken (ascending).  Sleeping components are the connected
    components of the sleepers (anything awake that touches one wakes it), over the edges of step 2 restricted to sleepers."""
    n = len(state)
    asleep = state["asleep"] != 0
    sensor = np.zeros(n, dtype=bool) if flags is None else (np.asarray(flags, dtype=np.uint32) & BODY_SENSOR) != 0
    pairs = [(int(m["body1"]), int(m["body2"])) for m in manifolds
             if int(m["point_count"]) > 0 and not sensor[int(m["body1"])] and not sensor[int(m["body2"])]]
    pairs += [(a, b) for a, b in units if b >= 0]
    label = labels(asleep, pairs)
    roots = {int(label[b]) for b in bodies_named if label[b] >= 0}
    woken = [i for i in range(n) if asleep[i] and int(label[i]) in roots]
    for i in woken:
        state["asleep"][i] = 0
        state["timer"][i] = F(0)
    return woken
