"""The reach of tests/solver_corpus.py, proven without a GPU: with the oracle's solver trace (oracle/phx_oracle.h PHXO_ST_*) every motif
takes the labels it is named for — in the reference's own order (solver_solve) and in the host builder's schedule (solver_solve_grouped),
in both arithmetic forms —, the corpus as a whole reaches every label of the trace, and the dressed path_edges cases reach the labels
stated for them.  The trace itself is held to its invariant first: a traced solve computes the bytes of an untraced one.

`pytest -s` prints the label table: a count per label for the corpus, beside the counts the scene and random inputs of the rest of the
suite give (the labels they never reach: tests/solver_corpus.py's reason to exist)."""
import itertools

import numpy as np
import pytest

import phyx_amd
import path_edges as pe
import solver_corpus as sc
from helpers import SMALL_SCENES, is_static, presolve_state
from test_solver_gpu import _random_state

ARITH = [0, 1]                    # oracle.ARITH_SOURCE, oracle.ARITH_FUSED


@pytest.fixture
def arith(request, oracle):
    prev = oracle.set_arith(request.param)
    yield request.param
    oracle.set_arith(prev)


def _host_schedule(state, island_mode=phyx_amd.ISLAND_MULTIPLE):
    """the host builder's schedule: (order, colour offsets, group offsets, LDS groups)"""
    bodies, _, joints = state
    args = (joints["body1"], joints["body2"], is_static(bodies), joints["contact_point_index"])
    if island_mode == phyx_amd.ISLAND_SINGLE:
        order, offs = phyx_amd.schedule_colours(*args)
        return order, offs, np.array([0, len(joints)], dtype=np.int32), 0
    g = phyx_amd.schedule_groups(*args)
    return g["order"], g["colour_offsets"], g["group_offsets"], g["lds_groups"]


def _grouped(oracle, state, sched, ci, pi, bits=32, trace=True):
    """the oracle's replay of a schedule -> (bodies, joints, stats, trace or None)"""
    b, cp, j = (a.copy() for a in state)
    order, offs, groups, lds = sched
    kw = dict(fp16_groups=lds) if bits == 16 else {}
    if not trace:
        return b, j, oracle.solver_solve_grouped(b, cp, j, order, offs, groups, ci, pi, oracle.STAG_COLOUR_SYNC, **kw), None
    with oracle.SolverTrace(len(j)) as tr:
        st = oracle.solver_solve_grouped(b, cp, j, order, offs, groups, ci, pi, oracle.STAG_COLOUR_SYNC, **kw)
    return b, j, st, tr


@pytest.fixture(autouse=True)
def _library(built_lib):
    """the host builder (phyx_amd.schedule_colours / schedule_groups) is the library's: built before any test here schedules"""


def _assert_motifs(corpus, tr, ci, pi, bits=32, skip=()):
    for name, copy, ji in corpus.instances:
        if name in skip:
            continue
        want, got = sc.motif_labels(name, ci, pi, bits), tr.joint_labels(ji)
        assert want <= got, "%r (copy %d) at (%d, %d), %d bits: not reached %s" % (name, copy, ci, pi, bits, sorted(want - got))


def _table(title, columns):
    """columns: [(heading, {label: count})]"""
    import oracle.binding as ob
    print("\n" + title)
    print("  %-20s" % "label" + "".join("%16s" % h for h, _ in columns))
    for l in ob.solver_trace_labels():
        print("  %-20s" % l + "".join("%16d" % c.get(l, 0) for _, c in columns))


def test_the_labels_are_the_corpus_files(oracle):
    names = oracle.solver_trace_labels()
    assert len(names) <= 64 and len(set(names)) == len(names)
    assert list(names) == sc.ALL_JOINT_LABELS + list(sc.HALF_LABELS) + list(sc.GROUP_LABELS)
    declared = set().union(*({sc._label(l)[0] for l in m[1]} | set(m[3]) for m in sc.MOTIFS.values()))
    assert set(sc.GPU_LEFT_OUT) <= set(sc.MOTIFS)
    assert declared <= set(names)
    assert all(1 <= len(sc.motif_alone(n).joints) <= 3 for n in sc.MOTIFS)
    assert all(len(sc.motif_alone(n).joints) == 3 for n in sc.CHAINS) and len(sc.CHAINS) >= 2


@pytest.mark.parametrize("arith", ARITH, indirect=True)
def test_how_long_a_motif_sweeps(oracle, arith):
    """What solver_corpus.GROUP_LABELS_ANY_GROUPING rests on: no motif alone but the deep chain runs more than two displacement sweeps;
    the deep chain runs DEEP_CHAIN_SWEEPS of them and one impulse sweep."""
    for name in sc.MOTIFS:
        perms = itertools.permutations(range(3)) if name in sc.CHAINS else [None]
        for perm in perms:
            c = sc.motif_alone(name, perm)
            b, cp, j = (a.copy() for a in c.state)
            st = oracle.solver_solve_ordered(b, cp, j, np.arange(len(j)), None, 12, 12)
            if name.startswith("deep chain"):
                assert st.displacement_iterations in sc.DEEP_CHAIN_SWEEPS and st.impulse_iterations == 1
            else:
                assert st.displacement_iterations <= 2, name


@pytest.mark.parametrize("arith", ARITH, indirect=True)
def test_a_traced_solve_computes_the_same_bytes(oracle, arith):
    """Marking a label changes nothing that is computed: through each of the four solve entry points, results with the trace on equal
    results with it off byte for byte (bodies, joints, every statistic), on the motifs, on a dressed case and on a random graph."""
    states = [sc.motifs().state, sc.dressed_state("tail", "static_spokes"), _random_state(np.random.default_rng(3), 300, 900, 0.1)]
    for state in states:
        single = _host_schedule(state, phyx_amd.ISLAND_SINGLE)
        multi = _host_schedule(state, phyx_amd.ISLAND_MULTIPLE)
        runs = {
            "solve": lambda b, cp, j: oracle.solver_solve(b, cp, j, oracle.SOLVE_AVX2, oracle.ISLAND_MULTIPLE, 6, 3)[1],
            "ordered": lambda b, cp, j: oracle.solver_solve_ordered(b, cp, j, single[0], single[1], 6, 3, oracle.STAG_SEQUENTIAL),
            "grouped": lambda b, cp, j: oracle.solver_solve_grouped(b, cp, j, multi[0], multi[1], multi[2], 3, 6, oracle.STAG_COLOUR_SYNC),
            "grouped_fp16": lambda b, cp, j: oracle.solver_solve_grouped(b, cp, j, multi[0], multi[1], multi[2], 6, 3, oracle.STAG_COLOUR_SYNC,
                                                                         fp16_groups=multi[3]),
        }
        for name, run in runs.items():
            out = []
            for traced in (False, True):
                b, cp, j = (a.copy() for a in state)
                if traced:
                    with oracle.SolverTrace(len(j)) as tr:
                        st = run(b, cp, j)
                    assert tr.reached and tr.masks.any(), name
                else:
                    st = run(b, cp, j)
                out.append((b.tobytes(), j.tobytes(), bytes(st)))
            assert out[0] == out[1], "the trace changed what %s computes" % name
    assert not oracle.lib().phxo_solver_get_trace()


@pytest.mark.parametrize("arith", ARITH, indirect=True)
def test_every_motif_takes_its_labels_and_the_corpus_takes_them_all(oracle, arith, capsys):
    """Every copy of every motif takes the labels it is named for (its other labels are not held against it: a joint always takes one
    label of each clamp) under solver_solve — Scalar (the packed modes skip eight joints or none, ref: Solver.cpp:798: what one joint of
    a pack is spared depends on its seven neighbours), Single and Multiple islands; a joint between two static bodies belongs to no
    island of GatherIslands (ref: Solver.cpp:367-379) and is only asked for in the Single mode — and under solver_solve_grouped on the
    host builder's schedule at every iteration count of the GPU tests.  The corpus as a whole reaches every per-joint label of the
    trace, the fp16 form the three half labels, and the four iteration counts over the two corpora together every per-group label.  Everything stays finite."""
    groups_seen = set()
    # (the whole corpus, the dynamic-only one, and the whole one as the GPU runs take it, without solver_corpus.GPU_LEFT_OUT: other
    #  contact-point ids, another schedule)
    for dynamic_only, leave_out in ((False, ()), (True, ()), (False, tuple(sc.GPU_LEFT_OUT))):
        corpus = sc.motifs(dynamic_only, leave_out=leave_out)
        assert sc.finite(corpus.bodies, corpus.joints)
        assert not dynamic_only or not is_static(corpus.bodies).any()
        names = {n for n, _, _ in corpus.instances}
        for island_mode in (oracle.ISLAND_SINGLE, oracle.ISLAND_MULTIPLE):
            b, cp, j = (a.copy() for a in corpus.state)
            with oracle.SolverTrace(len(j)) as tr:
                oracle.solver_solve(b, cp, j, oracle.SOLVE_SCALAR, island_mode, 6, 3)
            assert sc.finite(b, j)
            _assert_motifs(corpus, tr, 6, 3, skip=sc.NO_ISLAND if island_mode == oracle.ISLAND_MULTIPLE else ())
        columns = []
        for island_mode in (phyx_amd.ISLAND_SINGLE, phyx_amd.ISLAND_MULTIPLE):
            sched = _host_schedule(corpus.state, island_mode)
            for ci, pi in sc.ITERS:
                b, j, st, tr = _grouped(oracle, corpus.state, sched, ci, pi)
                assert sc.finite(b, j)
                _assert_motifs(corpus, tr, ci, pi)
                assert sc.corpus_labels(names, ci, pi) | sc.GROUP_LABELS_ANY_GROUPING[(ci, pi)] <= tr.reached
                if island_mode == phyx_amd.ISLAND_MULTIPLE:
                    columns.append(("ci %d, pi %d" % (ci, pi), tr.counts))
                    groups_seen |= tr.reached & set(sc.GROUP_LABELS)
        if not dynamic_only:
            assert sc.corpus_labels(names, 6, 3) == set(sc.ALL_JOINT_LABELS)            # no per-joint label is left out, GPU runs included
        else:
            assert sc.corpus_labels(names, 6, 3) == {l for l in sc.ALL_JOINT_LABELS if not l.startswith(("static_", "cim"))}
        # the fp16 form: every group the island kernel would take keeps its bodies in halves
        sched = _host_schedule(corpus.state)
        for ci, pi in sc.ITERS:
            b, j, st, tr = _grouped(oracle, corpus.state, sched, ci, pi, bits=16)
            assert sc.finite(b, j)
            assert sc.largest_body_word(corpus.bodies) < 6e4 and sc.largest_body_word(b) < 6e4      # every word stored, going in and coming out
            _assert_motifs(corpus, tr, ci, pi, bits=16)
            assert set(sc.HALF_LABELS) <= tr.reached
        columns.append(("fp16 6, 3", _grouped(oracle, corpus.state, sched, 6, 3, bits=16)[3].counts))
        with capsys.disabled():
            _table("solver corpus, %s motifs, host schedule (Multiple), arithmetic form %d: visits per label"
                   % ("dynamic-only" if dynamic_only else "all" if not leave_out else "all but the GPU runs' left-out", arith), columns)
    assert groups_seen == set(sc.GROUP_LABELS), sorted(set(sc.GROUP_LABELS) - groups_seen)


@pytest.mark.parametrize("arith", ARITH, indirect=True)
@pytest.mark.parametrize("name", sc.CHAINS)
def test_a_chain_takes_its_labels_under_every_permutation(oracle, arith, name):
    """The three-joint motifs do not depend on where a sweep visits their joints: all six orders, at every iteration count."""
    for perm in itertools.permutations(range(3)):
        for ci, pi in sc.ITERS:
            c = sc.motif_alone(name, perm)
            b, cp, j = (a.copy() for a in c.state)
            with oracle.SolverTrace(3) as tr:
                oracle.solver_solve_ordered(b, cp, j, np.arange(3), None, ci, pi)
            want = sc.motif_labels(name, ci, pi)
            assert want <= tr.reached, (perm, ci, pi, sorted(want - tr.reached))


@pytest.mark.parametrize("arith", ARITH, indirect=True)
def test_a_static_bodys_negative_zero_words_turn_positive_in_the_reference_order(oracle, arith):
    """solver_corpus.STATIC_NEGZERO, the motif the GPU parity runs leave out: the oracle, like the reference, stores word + 0 * impulse
    into a static body, and the first positive-zero product turns a -0.0 word into +0.0 — velocity.y with the first impulse sweep,
    displacing_velocity.y with the first displacement sweep; nothing else of the static body changes."""
    for ci, pi in sc.ITERS:
        c = sc.motif_alone(sc.STATIC_NEGZERO)
        b, cp, j = (a.copy() for a in c.state)
        assert is_static(b)[1] and b["velocity"]["y"][1:].view(np.uint32)[0] == 0x80000000
        assert b["displacing_velocity"]["y"][1:].view(np.uint32)[0] == 0x80000000
        oracle.solver_solve_ordered(b, cp, j, np.arange(1), None, ci, pi)
        assert b["velocity"]["y"][1:].view(np.uint32)[0] == 0
        assert b["displacing_velocity"]["y"][1:].view(np.uint32)[0] == (0 if pi else 0x80000000)
        kept = c.bodies.copy()
        kept["velocity"]["y"][1], kept["displacing_velocity"]["y"][1] = b["velocity"]["y"][1], b["displacing_velocity"]["y"][1]
        assert kept[1:].tobytes() == b[1:].tobytes()


@pytest.mark.parametrize("arith", ARITH, indirect=True)
@pytest.mark.parametrize("case", list(sc.DRESSED_CASES), ids=lambda c: "-".join(c))
def test_a_dressed_case_reaches_its_labels_and_keeps_its_design(oracle, arith, case):
    """dress() changes values only: the host builder's schedule of the dressed state is the undressed one's (so the class sizes, parts and
    group shapes tests/test_path_edges_cpu.py checks still hold), and its replay reaches the labels stated for the case."""
    kind, name = case
    plain = {"lds": pe.lds_state, "tail": pe.tail_state, "parts": pe.parts_state}[kind](name)
    state = sc.dressed_state(kind, name)
    for f in ("body1", "body2", "contact_point_index"):
        assert np.array_equal(state[2][f], plain[2][f])
    assert np.array_equal(is_static(state[0]), is_static(plain[0]))
    island_mode = phyx_amd.ISLAND_MULTIPLE if kind == "lds" else phyx_amd.ISLAND_SINGLE
    sched, plain_sched = _host_schedule(state, island_mode), _host_schedule(plain, island_mode)
    assert all(np.array_equal(a, b) for a, b in zip(sched[:3], plain_sched[:3])) and sched[3] == plain_sched[3]
    on_static = is_static(state[0])[state[2]["body1"]] | is_static(state[0])[state[2]["body2"]]
    assert on_static.any() == ("static_moving" in sc.DRESSED_CASES[case])
    for ci, pi in sc.DRESSED_ITERS:
        b, j, st, tr = _grouped(oracle, state, sched, ci, pi)
        assert sc.finite(b, j)
        want = sc.dressed_labels(case, ci, pi)
        assert want <= tr.reached, sorted(want - tr.reached)
    if kind == "lds":               # the fp16 form: the same labels but solver_corpus.DRESSED_DROP16, and the three half labels
        b, j, st, tr = _grouped(oracle, state, sched, 6, 3, bits=16)
        assert sc.finite(b, j) and sc.largest_body_word(state[0]) < 6e4 and sc.largest_body_word(b) < 6e4
        want = sc.dressed_labels(case, 6, 3, bits=16)
        assert want <= tr.reached, sorted(want - tr.reached)


def test_what_the_earlier_inputs_reach(oracle, capsys):
    """The baseline: the same counts for the world scenes (helpers.SMALL_SCENES) and the random graphs of tests/test_solver_gpu.py, in the
    reference's own order and on the host schedule, both arithmetic forms added up — printed beside the corpus, with the labels that only
    the corpus reaches.  (The scenes' displacing velocities: whatever the trace says under disp_in_*.)"""
    def add(total, counts):
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v

    def run(states, total):
        for state in states:
            multi = _host_schedule(state)
            for a in ARITH:
                prev = oracle.set_arith(a)
                try:
                    b, cp, j = (x.copy() for x in state)
                    with oracle.SolverTrace(len(j)) as tr:
                        oracle.solver_solve(b, cp, j, oracle.SOLVE_AVX2, oracle.ISLAND_MULTIPLE, 15, 15)
                    add(total, tr.counts)
                    add(total, _grouped(oracle, state, multi, 15, 15)[3].counts)
                    add(total, _grouped(oracle, state, multi, 15, 15, bits=16)[3].counts)
                finally:
                    oracle.set_arith(prev)

    scenes, random, corpus = {}, {}, {}
    run([presolve_state(make(), warm) for make, warm in SMALL_SCENES.values()], scenes)
    rng = np.random.default_rng(1)
    run([_random_state(rng, 4000, 3000, 0.05), _random_state(rng, 600, 6000, 0.05), _random_state(rng, 3000, 4000, 0.7),
         _random_state(rng, 3000, 6000, 0.1, units=True), pe.lds_state("units_256"), pe.tail_state("tail_of_3"), pe.tail_state("static_spokes")], random)
    run([sc.motifs().state], corpus)
    only = [l for l in oracle.solver_trace_labels() if corpus.get(l) and not scenes.get(l) and not random.get(l)]
    with capsys.disabled():
        _table("visits per label: the world scenes, the random and path_edges graphs, the motif corpus (ci = pi = 15)",
               [("scenes", scenes), ("random", random), ("corpus", corpus)])
        print("  reached by the corpus only: " + ", ".join(only))
    # what this corpus was written for: values that neither the scenes nor the random graphs carry
    assert {"static_moving", "disp_in_nonzero", "disp_in_negzero", "f_force_negzero", "i_subnormal", "d_subnormal"} <= set(only)
