"""Sleeping (include/phyx_amd.h SLEEPING; the definition: tests/sleep_spec.py) without a GPU: the rule on the CPU oracle's arithmetic,
every arm of the rule on fabricated states, and what the entry points and wrappers refuse before any device is needed.

The rest speeds the tolerances come from, measured on OracleWorld, scenes.tilted(12), gravity -200, dt 1/60, scalar, ISLAND_SINGLE,
15 + 15 iterations, steps 175 .. 400: the fastest body of the resting pile stays at |v| = 0.182 .. 0.198 and |w| = 0.0088 .. 0.0149 and
never gets quieter.  The tolerances 0.5 and 0.05 are about 2.5 x the linear and 3.4 x the angular rest speed."""
import ctypes as C

import numpy as np
import pytest

from phyx_amd import scenes
from phyx_amd.api import manifold_dtype, pin_dtype

import sleep_oracle
import sleep_spec

F = np.float32
PILE = list(range(1, 13))      # tilted(12): body 0 is the ground
BOX = 13


@pytest.fixture(scope="module")
def run(oracle):
    return sleep_oracle.run(oracle, scenes.tilted(12), 520)


def test_the_whole_pile_falls_asleep(run):
    before_box = run[:sleep_oracle.BOX_STEP]
    assert any(all(r["state"]["asleep"][i] for i in PILE) for r in before_box)
    assert not any(r["state"]["asleep"][0] for r in run)                   # the ground is static, not asleep
    assert not any(r["woken"] for r in before_box)                         # nothing touches a pile that rests


def test_a_sleeper_does_not_move(run):
    held = {}
    checked = 0
    for r in run:
        for i in range(len(r["state"])):
            if not r["state"]["asleep"][i]:
                held.pop(i, None)
                continue
            b = r["bodies"][i]
            now = tuple(b[f].tobytes() for f in ("pos", "xv", "yv", "aabb_min", "aabb_max"))
            assert b["inv_mass"] == 0 and b["inv_inertia"] == 0 and b["velocity"]["x"] == 0 and b["velocity"]["y"] == 0 and b["angular_velocity"] == 0
            if i in held:
                assert now == held[i], "body %d moved in its sleep" % i
                checked += 1
            held[i] = now
    assert checked > 1000


def test_the_dropped_box_wakes_part_of_the_pile(run):
    asleep_before = {i for i in PILE if run[sleep_oracle.BOX_STEP - 1]["state"]["asleep"][i]}
    assert asleep_before == set(PILE)
    first = next(r for r in run[sleep_oracle.BOX_STEP:] if r["woken"])
    woken = set(first["woken"])
    assert woken and woken < set(PILE)                                     # a non-empty proper subset: the component it hit
    assert all(first["state"]["asleep"][i] for i in set(PILE) - woken)


def test_timers_reset_on_wake(run):
    seen = 0
    for r in run:
        for i in r["woken"]:
            assert r["state"]["timer"][i] == 0 and not r["state"]["asleep"][i]
            assert r["bodies"]["inv_mass"][i] == r["state"]["inv_mass"][i] != 0      # its own masses are back
            seen += 1
    assert seen
    first = next(r for r in run[sleep_oracle.BOX_STEP:] if r["woken"])
    assert first["state"]["timer"][BOX] == 0                               # the whole component's timers, the waker's too


# ---- every arm of the rule on fabricated states ----------------------------------------------------------------------------------
def _state(n, asleep=(), timers=None):
    s = sleep_spec.new_state(n)
    for i in asleep:
        s["asleep"][i] = 1; s["inv_mass"][i] = 2.0; s["inv_inertia"][i] = 3.0
    if timers is not None:
        s["timer"] = np.asarray(timers, dtype=np.float32)
    return s


def _manifolds(*rows):
    m = np.zeros(len(rows), dtype=manifold_dtype)
    for k, (a, b, pc) in enumerate(rows):
        m[k] = (a, b, pc, 2 * k)
    return m


def _decide(state, masses, vel=None, manifolds=(), units=(), flags=None, params=(1.0, 1.0, 0.5), dt=0.25):
    n = len(state)
    masses = np.asarray(masses, dtype=np.float32).reshape(n, 2)
    vel = np.zeros((n, 3), dtype=np.float32) if vel is None else np.asarray(vel, dtype=np.float32).reshape(n, 3)
    m = _manifolds(*manifolds)
    return sleep_spec.decide(state, masses[:, 0], masses[:, 1], vel[:, 0], vel[:, 1], vel[:, 2], m, list(units), flags, sleep_spec.Params(*params), dt)


def test_a_unit_alone_is_an_edge():
    s = _state(3, timers=[0.5, 0.5, 0.0])
    slept, _ = _decide(s, [[1, 1]] * 3, vel=[[0, 0, 0], [0, 0, 0], [5, 0, 0]], units=[(0, 1)])
    assert slept == [0, 1]                                                 # 0 - 1 by the unit, calm; 2 on its own, moving
    s = _state(3, timers=[0.5, 0.5, 0.0])
    slept, _ = _decide(s, [[1, 1]] * 3, vel=[[0, 0, 0], [0, 0, 0], [5, 0, 0]], units=[(1, 2)])
    assert slept == [0]                                                    # 1 hangs on the moving 2: min timer 0


def test_a_unit_to_the_world_is_no_edge():
    s = _state(2, timers=[0.5, 0.0])
    slept, _ = _decide(s, [[1, 1]] * 2, vel=[[0, 0, 0], [5, 0, 0]], units=[(0, -1), (1, -1)])
    assert slept == [0]                                                    # both hang from the world: that links nothing


def test_a_sensor_manifold_is_no_edge():
    vel = [[0, 0, 0], [5, 0, 0]]
    s = _state(2, timers=[0.5, 0.0])
    assert _decide(s, [[1, 1]] * 2, vel=vel, manifolds=[(0, 1, 1)], flags=[0, 1])[0] == [0]
    s = _state(2, timers=[0.5, 0.0])
    assert _decide(s, [[1, 1]] * 2, vel=vel, manifolds=[(0, 1, 1)], flags=[0, 0])[0] == []


def test_a_manifold_without_points_is_no_edge():
    s = _state(2, timers=[0.5, 0.0])
    assert _decide(s, [[1, 1]] * 2, vel=[[0, 0, 0], [5, 0, 0]], manifolds=[(0, 1, 0)])[0] == [0]
    s = _state(2, asleep=[0])
    assert _decide(s, [[0, 0], [1, 1]], manifolds=[(0, 1, 0)])[1] == []   # ... and wakes nobody


def test_a_moving_static_strikes_and_a_still_one_does_not():
    for v, want in (([0, 0, 0], []), ([3, 0, 0], [0]), ([0, 0, 0.5], [0]), ([0, -0.0, 0], [0])):      # (any nonzero word moves: -0.0 too)
        s = _state(2, asleep=[0])
        _, woken = _decide(s, [[0, 0], [0, 0]], vel=[[0, 0, 0], v], manifolds=[(0, 1, 2)])
        assert woken == want, v
        assert s["asleep"][0] == (0 if want else 1)


def test_an_awake_body_wakes_the_whole_sleeping_component():
    s = _state(4, asleep=[0, 1, 3], timers=[0.7, 0.7, 0.3, 0.7])
    _, woken = _decide(s, [[0, 0], [0, 0], [1, 1], [0, 0]], manifolds=[(0, 1, 1), (1, 2, 1)])
    assert woken == [0, 1] and s["asleep"].tolist() == [0, 0, 0, 1]
    assert s["timer"].tolist() == [0, 0, 0, F(0.7)]                        # timer = 0 for the whole component, the waker's too


def test_a_pinned_body_is_dynamic():
    s = _state(1, timers=[0.25])                                           # inv_mass 0, inv_inertia > 0: it turns, so it can sleep
    slept, _ = _decide(s, [[0, 0.5]])
    assert slept == [0] and s["inv_mass"][0] == 0 and s["inv_inertia"][0] == F(0.5)
    s = _state(1)                                                          # a static body never does
    assert _decide(s, [[0, 0]]) == ([], []) and s["timer"][0] == 0


def test_the_timer_tie_sleeps():
    s = _state(1, timers=[0.25])
    assert _decide(s, [[1, 1]], params=(1.0, 1.0, 0.5), dt=0.25)[0] == [0]      # 0.25 + 0.25 == time_to_sleep
    s = _state(1, timers=[0.25])
    assert _decide(s, [[1, 1]], params=(1.0, 1.0, np.nextafter(F(0.5), F(1))), dt=0.25)[0] == []


def test_zero_tolerance_and_a_negative_zero_velocity():
    s = _state(1)
    _decide(s, [[1, 1]], vel=[[-0.0, 0.0, -0.0]], params=(0.0, 0.0, 10.0), dt=0.25)
    assert s["timer"][0] == F(0.25)                                        # (-0)(-0) = +0 <= 0: calm
    _decide(s, [[1, 1]], vel=[[1e-30, 0.0, 0.0]], params=(0.0, 0.0, 10.0), dt=0.25)
    assert s["timer"][0] == F(0.5)                                         # the square underflows to 0: calm by the rule as written
    _decide(s, [[1, 1]], vel=[[1e-10, 0.0, 0.0]], params=(0.0, 0.0, 10.0), dt=0.25)
    assert s["timer"][0] == 0


def test_labels_are_the_smallest_body():
    mobile = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    assert sleep_spec.labels(mobile, [(5, 4), (4, 1), (3, 2), (0, 2)]).tolist() == [0, 1, -1, 3, 1, 1]


def test_wake_components_wakes_connected_sleepers_only():
    s = _state(5, asleep=[0, 1, 2, 4])
    woken = sleep_spec.wake_components(s, [1], _manifolds((0, 1, 1), (1, 3, 1), (3, 4, 1), (2, 4, 0)), [])
    assert woken == [0, 1] and s["asleep"].tolist() == [0, 0, 1, 0, 1]


def test_unit_pairs_reads_every_kind():
    pins = np.zeros(2, dtype=pin_dtype)
    pins["body1"] = [3, 4]; pins["body2"] = [-1, 5]
    assert sleep_spec.unit_pairs([pins, None, np.zeros(0, dtype=pin_dtype)]) == [(3, -1), (4, 5)]


# ---- the entry points and the wrappers --------------------------------------------------------------------------------------------
def test_null_handle_is_an_error(built_lib):
    L = built_lib
    p = np.array([0.5, 0.05, 0.5], dtype=np.float32)
    on = C.c_int32(0)
    assert L.phx_world_set_sleeping(None, p.ctypes.data_as(C.c_void_p)) == -1
    assert L.phx_world_get_sleeping(None, p.ctypes.data_as(C.c_void_p), C.byref(on)) == -1
    assert L.phx_world_get_sleep_states(None, None, 0) == -1
    assert L.phx_world_wake_bodies(None, None, 0) == -1
    assert L.phx_world_sleep_counts(None, None, None, None) == -1
    assert b"null handle" in L.phx_last_error()


def test_set_sleeping_wants_all_three_or_none():
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = None, None
    with pytest.raises(ValueError):
        w.set_sleeping(0.5, 0.05)
    with pytest.raises(ValueError):
        w.set_sleeping(time_to_sleep=1.0)
