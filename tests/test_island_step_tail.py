"""The end of the island kernel's class step (island_kernel_body.h half_step): body stores first, the sweep's flag and the static tags by
address selection (spare words nobody reads), the ground wave's skip test as two unsigned compares per tag table, and one sweep loop
per kind of wave.  None of it may change a bit: every case is the device against the oracle replaying the device's own schedule —
velocities, displacing velocities, accumulated normal and friction impulses, byte for byte, in the arithmetic form the library states.

The shapes are the smallest at which the touched paths exist; that they do is checked on the CPU with the host schedule builder
(`_facts`) before anything runs on the device: three or more classes in a group, a wave with a unit on a static body, a working
wave without one, and for the two-static-bodies case lanes whose FIRST body is static and lanes whose SECOND is in the same wave,
with a two-joint unit on the (ground, box) pair.  Worlds are stepped 3 times before capture, as bench.py does (duplicate manifolds:
classes 3 and 4 exist)."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import scenes, Configuration
from helpers import is_static, presolve_state
from test_solver_gpu import _device_solve, _oracle_in_device_order

pytestmark = pytest.mark.gpu

WARM = 3


def _cfg(ci, pi, mode=phyx_amd.ISLAND_SINGLE_SLOPPY):      # (bench.py's configuration: the LDS groups)
    return Configuration(phyx_amd.SOLVE_AVX2, mode, ci, pi)


def _facts(state, lanes=256, cap=768):
    """What the host builder's schedule says about the shape: classes of the fullest group, waves with a unit on a static body, working
    waves without one, waves holding both a lane whose body 1 is static and a lane whose body 2 is, two-joint units on a static body."""
    bodies, _, joints = state
    st = is_static(bodies).astype(bool)
    hs = phyx_amd.schedule_groups(joints["body1"], joints["body2"], st, joints["contact_point_index"], lanes=lanes, body_cap=cap)
    slot, lane = hs["unit_leader_slot"], hs["unit_lane"]
    grp = np.searchsorted(hs["group_offsets"], slot, side="right") - 1
    cls = np.searchsorted(hs["colour_offsets"], slot, side="right") - 1
    lead = hs["order"][slot]
    s1, s2 = st[joints["body1"][lead]], st[joints["body2"][lead]]
    wave = grp * (lanes // 64) + lane // 64
    ws = np.unique(wave[s1 | s2])
    plain = np.setdiff1d(np.unique(wave), ws)
    both = np.intersect1d(np.unique(wave[s1]), np.unique(wave[s2]))
    pair = joints["body1"].astype(np.int64) * len(bodies) + joints["body2"]
    on_static = st[joints["body1"]] | st[joints["body2"]]
    _, per_pair = np.unique(pair[on_static], return_counts=True)
    classes = max(len(np.unique(cls[grp == g])) for g in np.unique(grp))
    return dict(lds_groups=hs["lds_groups"], groups=len(hs["group_offsets"]) - 1, classes=classes, ws_waves=len(ws), plain_waves=len(plain),
                st1_and_st2_waves=len(both), static_units_of_two=int((per_pair >= 2).sum()), units=len(slot), joints=len(joints))


def _two_static_scene():
    """stack(3, 70) with box 35 of every column static (zero inverse mass and inertia): the boxes above rest on it, the one below
    touches it from underneath — so the static body is body 1 of some units and body 2 of others, in one group."""
    sc = scenes.stack(3, 70)
    for col in range(3):
        sc["static"][1 + col * 70 + 35] = True
    return sc


_STATES = {}


def _state(name):
    """The captured solver inputs of a case: computed once, shared, never modified (every user copies)."""
    if name not in _STATES:
        scene = {"stack3x70": lambda: scenes.stack(3, 70), "two_static": _two_static_scene, "stack2x70": lambda: scenes.stack(2, 70),
                 "stack2x300": lambda: scenes.stack(2, 300)}[name]()
        _STATES[name] = presolve_state(scene, WARM, iters=20)
    return _STATES[name]


def _check_shape(name, lanes=256, cap=768, two_static=False):
    f = _facts(_state(name), lanes, cap)
    assert f["lds_groups"] == f["groups"] and f["lds_groups"] >= 1, f
    assert f["classes"] >= 3 and f["ws_waves"] >= 1 and f["plain_waves"] >= 1 and f["static_units_of_two"] >= 1, f
    if two_static:
        assert f["st1_and_st2_waves"] >= 1, f
    return f


@pytest.fixture(scope="module")
def solver(built_lib):
    return phyx_amd.Solver(0)


def _bit_exact(solver, oracle, state, cfg, fp16=False):
    gb, gj, sched, _, st = _device_solve(solver, state, cfg)
    assert sched.lds_groups == len(sched.groups) - 1, "some group left the island kernel"
    if fp16:
        ob_, cp, oj = (a.copy() for a in state)
        oracle.solver_solve_grouped(ob_, cp, oj, sched.order, sched.colours, sched.groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount,
                                    oracle.STAG_COLOUR_SYNC, fp16_groups=sched.lds_groups)
    else:
        ob_, oj, ost = _oracle_in_device_order(oracle, state, sched, None, cfg, oracle.STAG_COLOUR_SYNC)
        assert st.impulse_iterations == ost.impulse_iterations and st.displacement_iterations == ost.displacement_iterations
    for field in ("velocity", "angular_velocity", "displacing_velocity", "displacing_angular_velocity"):
        assert gb[field].tobytes() == ob_[field].tobytes(), "%s differs from the oracle" % field
    assert gb.tobytes() == ob_.tobytes(), "bodies differ from the oracle"
    for field in ("normal_acc", "friction_acc"):
        assert gj[field].tobytes() == oj[field].tobytes(), "%s differs from the oracle" % field
    assert gj.tobytes() == oj.tobytes(), "joints differ from the oracle"
    return gb, gj, st


@pytest.mark.parametrize("iters", [(20, 20), (20, 0), (0, 5), (1, 1)])
def test_stack3x70_bit_exact(solver, oracle, iters):
    """Cases 1 and 2: one ground wave and plain working waves in a group; (20, 20) leaves the two-half loop for the impulse-only loop
    after the first sweep, (20, 0) is the impulse-only loop alone, (0, 5) the displacement half alone, (1, 1) the two-half first sweep."""
    _check_shape("stack3x70")
    gb, gj, st = _bit_exact(solver, oracle, _state("stack3x70"), _cfg(*iters))
    if iters[0] == 20:
        assert 1 < st.impulse_iterations <= 20


def test_two_static_bodies_in_one_wave(solver, oracle):
    """Case 3: a static box mid-column beside the ground — lanes whose first body is static and lanes whose second is, in one wave, two
    static tags raised through atomicMax in one class step, and a two-joint unit on the (ground, box) pair whose follower must see the
    ground's record untouched."""
    _check_shape("two_static", two_static=True)
    _bit_exact(solver, oracle, _state("two_static"), _cfg(20, 20))


def test_material_table_set_world_follows_the_spec(oracle, built_lib):
    """Case 4: k_solve_islands_mat (same kernel body) — stack(2, 70) as a world with non-default friction and restitution on a few
    bodies, stepped against the oracle World under tests/material_spec.py's solve on the device's schedule, byte for byte."""
    import material_spec as spec
    from helpers import oracle_world
    from spawn_lockstep import compare
    from test_materials_gpu import _spec_step, _all
    _check_shape("stack2x70")
    sc = scenes.stack(2, 70)
    pw = phyx_amd.World(0, gravity=-200.0)
    pw.add_scene(sc)
    ow = oracle_world(sc)
    n = pw.counts()[0]
    f, e = np.full(n, 0.3, dtype=np.float32), np.zeros(n, dtype=np.float32)
    f[[1, 5, 71, 100]] = (0.0, 0.8, 1.0, 0.05)
    e[[2, 5, 71, 139]] = (0.8, 0.2, 0.5, 0.9)
    mat = spec.materials(n, f, e)
    pw.set_materials(_all(pw), mat["friction"], mat["restitution"])
    cfg = _cfg(20, 20, phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    for s in range(WARM + 2):
        _spec_step(oracle, pw, ow, cfg, mat)
        compare(pw, ow, s)
    groups, lds = pw.solver.groups()
    assert lds == len(groups) - 1 and lds >= 1, "the world's solve left the island kernel"


def test_stack2x300_uses_the_512_lane_shape(solver, oracle):
    """Case 5: columns of 300 boxes take k_solve_islands<512, 1024>; fp32 body state, then the fp16 body-state form of the same scene
    against the oracle's rounding model (k_solve_islands<512, 1024, true>)."""
    _check_shape("stack2x300", lanes=512, cap=1024)
    state = _state("stack2x300")
    gb, gj, st = _bit_exact(solver, oracle, state, _cfg(20, 20))
    s16 = phyx_amd.Solver(0)
    s16.set_body_state_bits(16)
    hb, hj, _ = _bit_exact(s16, oracle, state, _cfg(20, 20), fp16=True)
    assert hb.tobytes() != gb.tobytes()


def test_same_input_twice_gives_the_same_bytes(solver):
    """Case 6: the unconditional stores to the spare words make nothing order-dependent."""
    state, cfg = _state("stack3x70"), _cfg(20, 20)
    a = _device_solve(solver, state, cfg)
    b = _device_solve(solver, state, cfg)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
