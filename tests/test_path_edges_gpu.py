"""Parity at the capacity constants that choose a solve's kernel path (MI355X).  The constructions (tests/path_edges.py, checked on the CPU
by tests/test_path_edges_cpu.py) land exactly on the edges of k_solve_tail, k_solve_colour's grid, the two part levels and the LDS group
shapes.  Every case must equal the oracle's replay of the device's schedule byte for byte (bodies, joints, both iteration counts, joint
visits), equal the twin solver with the path switched off, and assert that it reached the edge it is about."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration
import path_edges as pe
from test_solver_gpu import _device_solve, _oracle_in_device_order

pytestmark = pytest.mark.gpu

ITERS = [(6, 3), (3, 6)]          # ci != pi both ways: the impulse-only and the displacement-only template instances run


def _solver(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = phyx_amd.Solver(0)
    for k in env:
        monkeypatch.delenv(k)
    return s


HANDED_OVER = "the device builder handed"      # csrc/solver_build.hip: printed (PHX_TRACE_SPEC=1) when a device build falls back to the host builder


def _solve_traced(solver, state, cfg, monkeypatch, capfd):
    """_device_solve with PHX_TRACE_SPEC=1 -> (its result, whether the device builder handed the build to the host builder)"""
    capfd.readouterr()
    monkeypatch.setenv("PHX_TRACE_SPEC", "1")
    try:
        out = _device_solve(solver, state, cfg)
    finally:
        monkeypatch.delenv("PHX_TRACE_SPEC")
    return out, HANDED_OVER in capfd.readouterr().err


def _oracle_parity(oracle, state, cfg, out, bits=32):
    """the device's solve (out = _device_solve's tuple) == the oracle's replay of its schedule, byte for byte"""
    gb, gj, sched, _, st = out
    if bits == 16:
        b, cp, j = (a.copy() for a in state)
        ost = oracle.solver_solve_grouped(b, cp, j, sched.order, sched.colours, sched.groups, cfg.contactIterationsCount,
                                          cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC, fp16_groups=sched.lds_groups)
        ob_, oj = b, j
    else:
        ob_, oj, ost = _oracle_in_device_order(oracle, state, sched, None, cfg, oracle.STAG_COLOUR_SYNC)
    assert gb.tobytes() == ob_.tobytes(), "bodies differ from the oracle"
    assert gj.tobytes() == oj.tobytes(), "joints differ from the oracle"
    assert (st.impulse_iterations, st.displacement_iterations, st.joint_visits) == (ost.impulse_iterations, ost.displacement_iterations, ost.joint_visits)
    return st


def _twin_parity(out, twin_out):
    """the twin solver (the path switched off) gives the same schedule and the same bytes"""
    gb, gj, sched, _, st = out
    tb, tj, tsched, _, tst = twin_out
    assert np.array_equal(tsched.order, sched.order) and np.array_equal(tsched.colours, sched.colours)
    assert tb.tobytes() == gb.tobytes() and tj.tobytes() == gj.tobytes()
    assert (tst.impulse_iterations, tst.displacement_iterations, tst.joint_visits) == (st.impulse_iterations, st.displacement_iterations, st.joint_visits)


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", list(pe.TAIL_CASES))
def test_tail_at_its_edges(oracle, built_lib, monkeypatch, capfd, name, iters):
    """k_solve_tail (csrc/solver_kernels.h; csrc/solver.hip tail_first_class): the HBM group's trailing classes of at most TAIL_T = 1024
    leaders, at most TAIL_CLASSES_MAX = 64 of them, in one workgroup's launch — lane t sweeps leader t (`tid < tab.y`) and follower t
    (`u < tab.z`), two classes per loop turn (odd and even nclass).  Cases: two classes of exactly 1024 leaders behind one of 1025 (every
    leader with a follower), tails of 2 and 3 classes (followers 0 in the last), a single qualifying class (no tail), 70 classes (> 64
    colours: the host builder, asserted by its PHX_TRACE_SPEC line; the tail capped at 64), units on a static body in every tail class.
    Asserted: the sweep launches are iterations x (the classes before the tail + one), the twin PHX_NO_TAIL=1 launches once per class and
    gives the same bytes."""
    leaders, followers, _, tail = pe.TAIL_CASES[name]
    state = pe.tail_state(name)
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, *iters)
    dev = phyx_amd.Solver(0)
    twin = _solver(monkeypatch, PHX_NO_TAIL="1")
    out, handed_over = _solve_traced(dev, state, cfg, monkeypatch, capfd)
    _, _, sched, _, st = out
    ki, parts, launches = dev.partition()
    L, F = pe.class_counts(sched.order, sched.colours, state[2])
    ncol = len(leaders)
    if name == "over_64_trailing":
        assert handed_over, "more than JP_MAX_COLOURS = 64 classes: the device builder must hand the build to the host builder"
    assert (L.tolist(), F.tolist()) == (leaders, followers) and st.colour_count == ncol and st.lds_islands == 0
    assert (ki, parts) == (0, 0) and launches == max(iters) * (tail + (1 if tail < ncol else 0))
    _oracle_parity(oracle, state, cfg, out)
    tout = _device_solve(twin, state, cfg)
    assert twin.partition()[2] == max(iters) * ncol
    _twin_parity(out, tout)


def test_tail_gates_the_displacement_sweeps(oracle, built_lib, monkeypatch):
    """k_solve_tail's `disp_on` gate (v.disp_active of the previous sweep): the displacement sweeps of a three-class tail stop being productive
    before pi, the launches still run and must skip them — displacement_iterations < pi, equal to the oracle and to PHX_NO_TAIL=1."""
    state = pe.tail_state("tail_of_3", shallow=True)
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, 3, 6)
    dev = phyx_amd.Solver(0)
    twin = _solver(monkeypatch, PHX_NO_TAIL="1")
    out = _device_solve(dev, state, cfg)
    assert dev.partition()[2] == 6 * 2
    st = _oracle_parity(oracle, state, cfg, out)
    assert 1 < st.displacement_iterations < 6
    _twin_parity(out, _device_solve(twin, state, cfg))


def test_colour_grid_past_one_pass(oracle, built_lib):
    """k_solve_colour's grid min(div_up(leaders, 64), 8192) and grid_for's min(div_up(n, 256), 2048) cover 524 288 items in one pass:
    one HBM class of exactly 524 289 leaders and one of 524 288, every leader with a follower (1 048 577 units, 2 097 154 joints), so that
    the grid-stride loops run a second pass for the last leader and its follower.  There is no switch for the stride (no twin): the oracle is
    the check, and the device schedule must have the designed classes."""
    state = pe.grid_state()
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, 2, 1)
    dev = phyx_amd.Solver(0)
    out = _device_solve(dev, state, cfg)
    _, _, sched, _, st = out
    L, F = pe.class_counts(sched.order, sched.colours, state[2])
    assert L.tolist() == pe.GRID_LEADERS and F.tolist() == pe.GRID_LEADERS and st.lds_islands == 0
    assert dev.partition() == (0, 0, 2 * 2)
    _oracle_parity(oracle, state, cfg, out)


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", list(pe.PARTS_CASES))
def test_parts_at_their_edges(oracle, built_lib, monkeypatch, capfd, name, iters):
    """The partitioned-component path (csrc/solver_kernels.h k_solve_parts_ahead at level 0, k_solve_parts at level 1, one
    launch per level and sweep; PARTS_CLASS_STRIDE = 64; csrc/schedule_kernels.h k_colour_parts, CP_MAXU = 3072).  Cases:
    lanes_256_257 — a body count that is not a multiple of 512 (the last level-0 part partial), level-0 classes of exactly 256 units (a
    perfect matching of a part's 512 bodies: every lane of PARTS_T = 256), level-1 parts of 256 units in all (200 + 56: every unit owned
    by a lane) and of 267 (200 + 57 + 10: the 257th in the middle of class 1, swept by the loop over `max(PARTS_T - before, 0) + tid`, and
    a class behind it where `before` > PARTS_T and the clamp holds the loop at the class's first unit); the first level-1 part (first
    body -256) is in the launch with nothing to sweep (no unit can be interior to it: tests/test_path_edges_cpu.py);
    over_64_interior_classes — more than 64 interior classes: the host builder, no part tables, every class swept by the class launches
    (and the tail); cp_maxu_3072 / 3073 — part 0 with exactly CP_MAXU interior units, coloured by the device builder, and one more, which
    the device builder hands to the host builder (both asserted by the PHX_TRACE_SPEC line of csrc/solver_build.hip).
    Equal to the oracle, to the host builder (PHX_SCHEDULE_BUILDER=host) and to PHX_NO_PARTS=1 PHX_NO_TAIL=1 (one launch per class)."""
    nb, sizes, star0, dense0 = pe.PARTS_CASES[name]
    state = pe.parts_state(name)
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, *iters)
    dev = phyx_amd.Solver(0)
    host = _solver(monkeypatch, PHX_SCHEDULE_BUILDER="host")
    plain = _solver(monkeypatch, PHX_NO_PARTS="1", PHX_NO_TAIL="1")
    out, handed_over = _solve_traced(dev, state, cfg, monkeypatch, capfd)
    _, _, sched, _, st = out
    ki, parts, launches = dev.partition()
    ncol = len(sched.colours) - 1
    P = (nb + pe.PART_BODIES - 1) // pe.PART_BODIES
    it = max(iters)
    seen = dict(classes=ncol, partition=(ki, parts, launches), handed_over=handed_over)
    assert st.lds_islands == 0, seen
    if name in ("over_64_interior_classes", "cp_maxu_3073"):
        assert handed_over, seen                    # > JP_MAX_COLOURS classes / > CP_MAXU units in a part: the host builder
    if name == "cp_maxu_3072":
        assert not handed_over, seen                # exactly CP_MAXU units in part 0: k_colour_parts coloured it
    if name == "over_64_interior_classes":
        L, _ = pe.class_counts(sched.order, sched.colours, state[2])
        assert ki > pe.PARTS_CLASS_STRIDE and parts == 0, seen
        t = pe.tail_first_class(L.tolist())
        assert launches == it * (t + (1 if t < ncol else 0)), seen
    else:
        levels1 = max(len(s) for s in sizes)
        assert ki == ncol and parts == 2 * P + 1 and launches == it * 2, seen      # every class interior: one launch per level
        assert ki - levels1 >= 1, seen
    _oracle_parity(oracle, state, cfg, out)
    hout = _device_solve(host, state, cfg)
    assert host.partition()[:2] == (ki, parts)
    _twin_parity(out, hout)
    pout = _device_solve(plain, state, cfg)
    assert plain.partition() == (ki, 0, it * ncol)
    _twin_parity(out, pout)


@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("name", list(pe.LDS_CASES))
def test_lds_group_shapes_at_their_edges(oracle, built_lib, monkeypatch, name, bits):
    """The LDS group shapes (csrc/island_view.h ISL_T / ISL_T_BIG = 256 / 512 lanes, i.e. units; joints twice that — COLOUR_B_MAX_JOINTS =
    1024 is the step to the HBM group) with body state at 32 and at 16 bits: a component of 256 units (512 joints) stays in the small
    shape, 257 units take the 512-lane shape, 512 units of 1024 joints fit it exactly, 513 units (513 or 1025 joints) go to the HBM group.
    (The body caps ISL_B / ISL_B_BIG cannot bind: tests/test_path_edges_cpu.py.)  Equal to the oracle (fp16_groups for 16 bits) and to the
    host builder (PHX_SCHEDULE_BUILDER=host)."""
    units, two, shape = pe.LDS_CASES[name]
    state = pe.lds_state(name)
    nj = len(state[2])
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_MULTIPLE, 6, 3)
    dev = phyx_amd.Solver(0)
    host = _solver(monkeypatch, PHX_SCHEDULE_BUILDER="host")
    if bits == 16:
        dev.set_body_state_bits(16)
        host.set_body_state_bits(16)
    out = _device_solve(dev, state, cfg)
    _, _, sched, _, st = out
    _, lane = dev.lanes()
    in_lds = int(sched.groups[sched.lds_groups])
    if shape == "hbm":
        assert nj - in_lds == units + two and st.lds_islands >= 1     # the path in the HBM group, the small islands in LDS
        assert lane.max() < pe.ISL_T
    else:
        assert in_lds == nj
        assert (lane.max() >= pe.ISL_T) == (shape == "big") and lane.max() < (pe.ISL_T_BIG if shape == "big" else pe.ISL_T)
    _oracle_parity(oracle, state, cfg, out, bits)
    _twin_parity(out, _device_solve(host, state, cfg))
