"""Solver parity on the directed joint values of tests/solver_corpus.py (MI355X): signed zeros, subnormals, caller-supplied displacing
velocities, moving static bodies, static bodies in every slot of a unit, warm starts on the clamps' edges, half stores that flush, tie
or go subnormal.  Every run must equal the oracle's replay of the device's own schedule byte for byte (bodies, joints, both iteration
counts, joint visits) and the host-builder or path-off twin; the replay runs under the oracle's solver trace, and every label the input
is built for (proven reachable on the CPU by tests/test_solver_corpus_cpu.py) is asserted reached on the DEVICE's schedule, so no run
passes by having gone somewhere else."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration
import path_edges as pe
import solver_corpus as sc
from helpers import is_static
from test_solver_gpu import _device_solve
from test_path_edges_gpu import _solver, _oracle_parity, _twin_parity

pytestmark = pytest.mark.gpu

# path -> (island mode, body state bits, environment of the solver)
PATHS = {
    "lds": (phyx_amd.ISLAND_MULTIPLE, 32, {}),                          # the LDS island kernel
    "lds_fp16": (phyx_amd.ISLAND_MULTIPLE, 16, {}),                     # ... with body state in halves
    "hbm": (phyx_amd.ISLAND_SINGLE, 32, {}),                            # the HBM colour kernels
    "no_islands": (phyx_amd.ISLAND_MULTIPLE, 32, {"PHX_NO_ISLANDS": "1"}),
}


@pytest.fixture(scope="module")
def corpora():
    return {False: sc.motifs(False, leave_out=sc.GPU_LEFT_OUT), True: sc.motifs(True, leave_out=sc.GPU_LEFT_OUT)}


def _traced_parity(oracle, state, cfg, out, bits=32):
    """_oracle_parity with the solver trace on in the replay -> (the device's stats, the trace)"""
    with oracle.SolverTrace(len(state[2])) as tr:
        st = _oracle_parity(oracle, state, cfg, out, bits)
    return st, tr


@pytest.mark.parametrize("iters", sc.ITERS, ids=lambda i: "ci%d_pi%d" % i)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dynamic_only", [False, True], ids=["all", "dynamic_only"])
def test_motifs(oracle, built_lib, monkeypatch, corpora, dynamic_only, path, iters):
    """The motif islands, whole and without the ones on static bodies (no wave of the island kernel then takes the static form of the
    class step), through the LDS island kernel at 32 and 16 bits of body state, the HBM colour kernels (ISLAND_SINGLE) and
    PHX_NO_ISLANDS=1, at sweep counts with ci > pi, ci < pi, one sweep each and no displacement sweeps."""
    island_mode, bits, env = PATHS[path]
    corpus = corpora[dynamic_only]
    state = corpus.state
    nj = len(state[2])
    ci, pi = iters
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, island_mode, ci, pi)
    dev = _solver(monkeypatch, **env)
    host = _solver(monkeypatch, PHX_SCHEDULE_BUILDER="host", **env)
    if bits == 16:
        dev.set_body_state_bits(16)
        host.set_body_state_bits(16)
    out = _device_solve(dev, state, cfg)
    gb, gj, sched, _, st = out
    assert sorted(sched.order.tolist()) == list(range(nj)) and sc.finite(gb, gj)
    if path.startswith("lds"):
        both_static = (is_static(state[0])[state[2]["body1"]] & is_static(state[0])[state[2]["body2"]]).astype(bool)
        assert st.lds_islands >= 1 and int(sched.groups[sched.lds_groups]) == nj - int(both_static.sum())      # every island in an LDS group
    else:
        assert st.lds_islands == 0
    _, tr = _traced_parity(oracle, state, cfg, out, bits)
    for name, copy, ji in corpus.instances:
        want, got = sc.motif_labels(name, ci, pi, bits), tr.joint_labels(ji)
        assert want <= got, "%r (copy %d): not reached on the device's schedule: %s" % (name, copy, sorted(want - got))
    names = {n for n, _, _ in corpus.instances}
    want = sc.corpus_labels(names, ci, pi, bits) | sc.GROUP_LABELS_ANY_GROUPING[iters] | (set(sc.HALF_LABELS) if bits == 16 else set())
    assert want <= tr.reached, sorted(want - tr.reached)
    _twin_parity(out, _device_solve(host, state, cfg))


@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_a_static_bodys_negative_zero_words_stay(oracle, built_lib, monkeypatch, path):
    """The stated deviation, pinned: the one motif test_motifs leaves out (solver_corpus.GPU_LEFT_OUT).  The
    reference stores word + 0 * impulse into a static body, which turns a -0.0 word into +0.0 with the first positive-zero product; the
    device never stores a static body's record.  Solved alone, five copies: every byte equals the oracle's replay but velocity.y and
    displacing_velocity.y of the static bodies, where the oracle has 0x00000000 and the device the 0x80000000 it was given."""
    c = sc._assemble([(sc.STATIC_NEGZERO, k) for k in range(sc.COPIES)], 3)
    state = c.state
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_MULTIPLE if path == "lds" else phyx_amd.ISLAND_SINGLE, 6, 3)
    dev = phyx_amd.Solver(0)
    gb, gj, sched, _, st = _device_solve(dev, state, cfg)
    assert (st.lds_islands >= 1) == (path == "lds")
    b, cp, j = (a.copy() for a in state)
    with oracle.SolverTrace(len(j)) as tr:
        ost = oracle.solver_solve_grouped(b, cp, j, sched.order, sched.colours, sched.groups, 6, 3, oracle.STAG_COLOUR_SYNC)
    for name, copy, ji in c.instances:
        assert sc.motif_labels(name, 6, 3) <= tr.joint_labels(ji)
    static = is_static(state[0]).astype(bool)
    for f in ("velocity", "displacing_velocity"):
        assert (b[f]["y"][static].view(np.uint32) == 0).all(), "the oracle's words"
        assert (gb[f]["y"][static].view(np.uint32) == 0x80000000).all(), "the device's words"
        b[f]["y"][static] = gb[f]["y"][static]                 # ... and with those words set aside,
    assert gb.tobytes() == b.tobytes() and gj.tobytes() == j.tobytes()      # every other byte is the oracle's
    assert (st.impulse_iterations, st.displacement_iterations, st.joint_visits) == (ost.impulse_iterations, ost.displacement_iterations, ost.joint_visits)


@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("name", ["units_256", "units_257"])
def test_dressed_lds_group_shapes(oracle, built_lib, monkeypatch, name, bits):
    """The path components at the small LDS shape's capacity and one unit past it (the 512-lane shape), re-valued by solver_corpus.dress:
    the shape assertions of tests/test_path_edges_gpu.py, the oracle, the host-builder twin, the case's labels."""
    units, two, shape = pe.LDS_CASES[name]
    state = sc.dressed_state("lds", name)
    nj = len(state[2])
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_MULTIPLE, 6, 3)
    dev = phyx_amd.Solver(0)
    host = _solver(monkeypatch, PHX_SCHEDULE_BUILDER="host")
    if bits == 16:
        dev.set_body_state_bits(16)
        host.set_body_state_bits(16)
    out = _device_solve(dev, state, cfg)
    gb, gj, sched, _, st = out
    _, lane = dev.lanes()
    assert int(sched.groups[sched.lds_groups]) == nj and sc.finite(gb, gj)
    assert (lane.max() >= pe.ISL_T) == (shape == "big") and lane.max() < (pe.ISL_T_BIG if shape == "big" else pe.ISL_T)
    _, tr = _traced_parity(oracle, state, cfg, out, bits)
    want = sc.dressed_labels(("lds", name), 6, 3, bits)
    assert want <= tr.reached, sorted(want - tr.reached)
    _twin_parity(out, _device_solve(host, state, cfg))


@pytest.mark.parametrize("iters", sc.DRESSED_ITERS, ids=lambda i: "ci%d_pi%d" % i)
@pytest.mark.parametrize("name", ["tail_of_3", "static_spokes"])
def test_dressed_tail(oracle, built_lib, monkeypatch, name, iters):
    """k_solve_tail on re-valued stars (static_spokes: every tail class holds units on a MOVING static body): the designed classes and
    launch counts of tests/test_path_edges_gpu.py, the oracle, the twin PHX_NO_TAIL=1, the case's labels."""
    leaders, followers, _, tail = pe.TAIL_CASES[name]
    state = sc.dressed_state("tail", name)
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, *iters)
    dev = phyx_amd.Solver(0)
    twin = _solver(monkeypatch, PHX_NO_TAIL="1")
    out = _device_solve(dev, state, cfg)
    gb, gj, sched, _, st = out
    ki, parts, launches = dev.partition()
    L, F = pe.class_counts(sched.order, sched.colours, state[2])
    ncol = len(leaders)
    assert (L.tolist(), F.tolist()) == (leaders, followers) and st.colour_count == ncol and st.lds_islands == 0 and sc.finite(gb, gj)
    assert (ki, parts) == (0, 0) and launches == max(iters) * (tail + (1 if tail < ncol else 0))
    _, tr = _traced_parity(oracle, state, cfg, out)
    want = sc.dressed_labels(("tail", name), *iters)
    assert want <= tr.reached, sorted(want - tr.reached)
    tout = _device_solve(twin, state, cfg)
    assert twin.partition()[2] == max(iters) * ncol
    _twin_parity(out, tout)


@pytest.mark.parametrize("iters", sc.DRESSED_ITERS, ids=lambda i: "ci%d_pi%d" % i)
def test_dressed_parts(oracle, built_lib, monkeypatch, iters):
    """The partitioned-component path (k_solve_parts_ahead, k_solve_parts) on lanes_256_257 re-valued: the part assertions of
    tests/test_path_edges_gpu.py, the oracle, the host builder and the twin PHX_NO_PARTS=1 PHX_NO_TAIL=1, the case's labels."""
    name = "lanes_256_257"
    nb, sizes, star0, dense0 = pe.PARTS_CASES[name]
    state = sc.dressed_state("parts", name)
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_SINGLE, *iters)
    dev = phyx_amd.Solver(0)
    host = _solver(monkeypatch, PHX_SCHEDULE_BUILDER="host")
    plain = _solver(monkeypatch, PHX_NO_PARTS="1", PHX_NO_TAIL="1")
    out = _device_solve(dev, state, cfg)
    gb, gj, sched, _, st = out
    ki, parts, launches = dev.partition()
    ncol = len(sched.colours) - 1
    P = (nb + pe.PART_BODIES - 1) // pe.PART_BODIES
    it = max(iters)
    assert st.lds_islands == 0 and sc.finite(gb, gj)
    assert ki == ncol and parts == 2 * P + 1 and launches == it * 2, (ki, ncol, parts, launches)
    _, tr = _traced_parity(oracle, state, cfg, out)
    want = sc.dressed_labels(("parts", name), *iters)
    assert want <= tr.reached, sorted(want - tr.reached)
    hout = _device_solve(host, state, cfg)
    assert host.partition()[:2] == (ki, parts)
    _twin_parity(out, hout)
    pout = _device_solve(plain, state, cfg)
    assert plain.partition() == (ki, 0, it * ncol)
    _twin_parity(out, pout)
