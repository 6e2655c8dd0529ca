"""The end of the island kernel's launch (MI355X): the solve's end stamp and the write-back of quiet groups.

Every workgroup of the island kernel leaves the clock at its end in one of a few words (csrc/solver_kernels.h solve_stamp_end) and the
host takes the maximum: phx_solve_stats.device_ms must cover the LAST group to finish, whichever word it stamped.  A group whose
displacement half is skipped leaves its displacing velocities alone (csrc/island_kernel_body.h, FinishBodies); a group that is not
quiet — by a deep joint or by a displacing velocity that is not +0, -0 included — must still write them."""
import time

import numpy as np
import pytest

import phyx_amd
from phyx_amd import scenes, Configuration
from helpers import is_static, presolve_state

pytestmark = pytest.mark.gpu

# Group counts are the schedule's, not the scene's: after three world steps a column is not yet one island, and the builder bins
# islands into 256-lane groups — stack(70, 130) comes out as 43 groups and stack(3, 130) as 2, stack(n, 200) as n or n + 1.  Every
# test asserts the count it relies on from solver.groups().
STAT_SLOTS, STAMP_WORDS = 64, 16      # csrc/solver_kernels.h ISL_STAT_SLOTS, STAMP_END_SHARDS
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)
TICK_MS = 1e-5               # the stamps' clock: 100 MHz


@pytest.fixture(scope="module")
def states():
    """solver inputs after three world steps and PreSolve, per scene: made once, never modified (the tests solve copies)"""
    made = {}

    def get(columns, rows):
        if (columns, rows) not in made:
            made[(columns, rows)] = presolve_state(scenes.stack(columns, rows), 3)
        return made[(columns, rows)]
    return get


def _solve_timed(solver, state, cfg=CFG):
    """one synchronised SolveJointsDevice of a copy of `state` -> (device arrays, stats, host wall time in ms)"""
    d = [phyx_amd.DeviceArray(a) for a in state]
    solver.synchronize()
    t0 = time.perf_counter()
    solver.SolveJointsDevice(d[0], d[1], d[2], cfg)
    solver.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t0)
    return d, solver.stats(), wall_ms


@pytest.mark.parametrize("columns,rows,groups", [(70, 200, 71), (70, 130, 43)])
def test_every_groups_end_reaches_the_stamp(built_lib, states, columns, rows, groups):
    """More groups than stamp words — 71: also more than stat slots —, so that every word receives several groups, solved in the trace
    instantiation: device_ms is at least the span from the start of block 0's group to the LATEST 'swept' stamp of any group — exact,
    the same 100 MHz clock, and the end stamp is read behind 'swept' — and at most the host's wall time of the call."""
    solver = phyx_amd.Solver(0)
    solver.set_trace(True, waves=False)
    _, st, wall_ms = _solve_timed(solver, states(columns, rows))
    _, lds_groups = solver.groups()
    assert lds_groups == groups and groups > STAMP_WORDS and (rows != 200 or groups > STAT_SLOTS)
    t = solver.island_trace().astype(np.int64)
    assert t.shape[0] == groups and (t[:, 0] != 0).all() and (t[:, 4] != 0).all()
    ticks = int(t[:, 4].max() - t[0, 0])
    assert ticks > 0
    # device_ms is the float32 of (end - begin) x 1e-5 with begin <= stamp 0 of block 0 and end >= every group's stamp 4: rounding is
    # monotonic, so the bound is compared in the same precision and stays exact
    lower = float(np.float32(ticks * TICK_MS))
    print("device_ms %.6f, latest swept - block 0's start %.6f ms (group %d), host wall %.3f ms" % (st.device_ms, lower, int(t[:, 4].argmax()), wall_ms))
    assert st.device_ms >= lower
    assert st.device_ms <= wall_ms


@pytest.mark.parametrize("columns,rows,groups", [(1, 20, 1), (16, 200, 16), (17, 200, 17), (63, 200, 64), (64, 200, 65)])
def test_device_ms_is_positive(built_lib, states, columns, rows, groups):
    """one group, and a group count at and one past the number of stamp words (16) and of stat slots (64); the first solve builds the
    schedule (the launch is gated by the build), the second one checks the cached schedule inside the island kernel"""
    solver = phyx_amd.Solver(0)
    for _ in range(2):
        _, st, wall_ms = _solve_timed(solver, states(columns, rows))
        assert solver.groups()[1] == groups
        assert 0.0 < st.device_ms <= wall_ms


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _group_bodies(sched_order, group_offsets, joints, g):
    j = joints[sched_order[group_offsets[g]:group_offsets[g + 1]]]
    return np.unique(np.concatenate([j["body1"], j["body2"]]))


@pytest.mark.parametrize("penetration_iterations", [20, 0])
@pytest.mark.parametrize("rows,groups", [(200, 3), (130, 2)])
def test_quiet_and_stirred_groups_in_one_launch(built_lib, oracle, states, rows, groups, penetration_iterations):
    """Groups of three kinds in one launch: the first has a box pushed 3 units into its neighbour (displacement sweeps run), the second
    a body with a displacing velocity of -0.0 (not quiet by the kernel's bit test), the third is left alone (quiet: its displacing
    velocities are not written back).  Everything the solve leaves must be the oracle's grouped replay of the exported schedule, bit
    for bit.  (stack(3, 130), 391 bodies, is two groups: it has the two stirred kinds only.)"""
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, penetration_iterations)
    base = states(3, rows)
    assert len(base[0]) == 3 * rows + 1
    # the schedule (a function of the joints alone) of the unmodified state: which joints and bodies each group holds
    probe = phyx_amd.Solver(0)
    _solve_timed(probe, base, cfg)
    order, _ = probe.schedule()
    goffs, lds_groups = probe.groups()
    assert lds_groups == groups
    b, cp, j = (a.copy() for a in base)
    static = is_static(b).astype(bool)
    # group 0: one box 3 units towards the box it touches
    k = next(int(q) for q in order[goffs[0]:goffs[1]] if not static[j["body1"][q]] and not static[j["body2"][q]])
    b1, b2 = int(j["body1"][k]), int(j["body2"][k])
    dx, dy = float(b["pos"]["x"][b2] - b["pos"]["x"][b1]), float(b["pos"]["y"][b2] - b["pos"]["y"][b1])
    n = (dx * dx + dy * dy) ** 0.5
    b["pos"]["x"][b1] += np.float32(3.0 * dx / n)
    b["pos"]["y"][b1] += np.float32(3.0 * dy / n)
    # group 1: -0.0 in one displacing velocity
    dyn1 = [int(x) for x in _group_bodies(order, goffs, j, 1) if not static[x]]
    b["displacing_velocity"]["x"][dyn1[len(dyn1) // 2]] = np.float32(-0.0)
    assert _bits(b["displacing_velocity"]["x"])[dyn1[len(dyn1) // 2]] == 0x80000000
    state = (b, cp, j)

    solver = phyx_amd.Solver(0)
    d, st, _ = _solve_timed(solver, state, cfg)
    gb, gj = d[0].to_host(), d[2].to_host()
    s_order, s_colours = solver.schedule()
    s_groups, s_lds = solver.groups()
    assert s_lds == groups
    ob_, ocp, oj = (a.copy() for a in state)
    ost = oracle.solver_solve_grouped(ob_, ocp, oj, s_order, s_colours, s_groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount,
                                      oracle.STAG_COLOUR_SYNC)
    for f in ("velocity", "displacing_velocity"):
        for c in ("x", "y"):
            assert np.array_equal(_bits(gb[f][c]), _bits(ob_[f][c])), "%s.%s differs from the oracle" % (f, c)
    for f in ("angular_velocity", "displacing_angular_velocity"):
        assert np.array_equal(_bits(gb[f]), _bits(ob_[f])), "%s differs from the oracle" % f
    for f in ("normal_acc", "friction_acc"):
        assert np.array_equal(_bits(gj[f]), _bits(oj[f])), "%s differs from the oracle" % f
    assert st.impulse_iterations == ost.impulse_iterations and st.displacement_iterations == ost.displacement_iterations
    # the scene is what it is meant to be: the third group stayed quiet, and with displacement sweeps the first one was pushed apart
    def dvel_bits(bodies):
        return _bits(ob_["displacing_velocity"]["x"])[bodies] | _bits(ob_["displacing_velocity"]["y"])[bodies] | _bits(ob_["displacing_angular_velocity"])[bodies]
    if groups > 2:
        quiet = [int(x) for x in _group_bodies(s_order, s_groups, j, 2) if not static[x]]
        assert len(quiet) > 0 and (dvel_bits(quiet) == 0).all()
    if penetration_iterations:
        stirred = [int(x) for x in _group_bodies(s_order, s_groups, j, 0) if not static[x]]
        assert (dvel_bits(stirred) != 0).any()
