"""The premises of the sleep corpus (tests/sleep_corpus.py) without a GPU: every case's components by a breadth-first search of its own
against sleep_spec's labels, the step in which every component falls asleep against sleep_spec.decide, that the edges exert nothing
(unit_spec on the oracle's records), the tie and the squares the `tie` and `zeros` cases stand on, the wave premise of
`interleaved_pairs`, and the scenes of Part B on the CPU oracle as far as the oracle carries them."""
import os
import re

import numpy as np
import pytest

from phyx_amd.api import manifold_dtype

import break_spec
import sleep_corpus as corpus
import sleep_oracle
import sleep_spec
import unit_spec
from sleep_corpus import DT, F, ksum, after

CASES = {c.name: c for c in corpus.graph_cases()}


@pytest.fixture(scope="module")
def runs():
    """per graph case (the spec's slept lists per step, the state after the last step, the steps)"""
    out = {}
    for name, case in CASES.items():
        steps = max(s for s in case.sleep_steps().values() if s is not None) + 3
        out[name] = corpus.simulate(case, ksum(case.k), steps) + (steps,)
    return out


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def test_every_clause_is_reached_by_a_case():
    table = corpus.table()
    for case, reaches in table.items():
        assert reaches and set(reaches) <= set(corpus.CLAUSES), case
    for clause in corpus.CLAUSES:
        assert any(clause in reaches for reaches in table.values()), "no case reaches: " + clause


def test_the_constants_are_the_kernels():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "phyx_amd", "csrc")
    text = open(os.path.join(csrc, "sleep_kernels.h")).read()
    assert int(re.search(r"SLEEP_WAVE_ROOTS\s*=\s*(\d+)", text).group(1)) == corpus.SLEEP_WAVE_ROOTS
    text = open(os.path.join(csrc, "schedule_kernels.h")).read()
    assert int(re.search(r"CCW_BODIES\s*=\s*(\d+)", text).group(1)) == corpus.CCW_BODIES


# ---- the graph cases: components and sleep steps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_spec_labels_are_the_breadth_first_components(name):
    case = CASES[name]
    comp = corpus.components(case.n, case.mobile(), case.pairs())
    want = np.full(case.n, -1, dtype=np.int64)
    for root, members in comp.items():
        want[members] = root
    assert sleep_spec.labels(case.mobile(), case.pairs()).tolist() == want.tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_spec_sleeps_each_component_in_its_step(name, runs):
    case = CASES[name]
    slept, state, steps = runs[name]
    assert slept == case.expected_slept(steps)
    never = [r for r, s in case.sleep_steps().items() if s is None]
    comp = corpus.components(case.n, case.mobile(), case.pairs())
    for r in never:
        assert not state["asleep"][comp[r]].any()


def test_the_shapes_of_the_graph_cases(runs):
    n = corpus.PATH_N
    assert corpus.components(n, np.ones(n, dtype=bool), CASES["permuted_path"].pairs()) == {0: list(range(n))}
    assert runs["permuted_path"][0][:3] == [[], [], list(range(n))]
    # cut_path: 601 and 899 bodies; the larger part holds the body that turns and stays awake with the timers the spec says
    case, order = CASES["cut_path"], corpus.path_order()
    comp = corpus.components(n, np.ones(n, dtype=bool), case.pairs())
    small, large = sorted(order[:corpus.PATH_CUT + 1]), sorted(order[corpus.PATH_CUT + 1:])
    assert sorted(comp.values(), key=len) == [small, large] and (len(small), len(large)) == (601, 899)
    spinner = order[corpus.PATH_SPINNER]
    assert spinner in large
    slept, state, steps = runs["cut_path"]
    assert slept[2] == small and sum(map(len, slept)) == len(small)
    rest = [b for b in large if b != spinner]
    assert state["timer"][spinner] == 0 and (state["timer"][rest] == ksum(steps)).all()
    # the stars: one component under body 0, the hub at either end of the indices
    for name, hub in (("star_high", 600), ("star_low", 0)):
        pairs = CASES[name].pairs()
        assert all(hub in p for p in pairs) and len(pairs) == 600
        assert corpus.components(601, np.ones(601, dtype=bool), pairs) == {0: list(range(601))}
        assert {p[0] == hub for p in pairs} == {True, False}
    # window_runs: every run is a component under its first body; lengths 255, 256, 257 at a window border and one past it
    comp = corpus.components(corpus.RUNS_N, np.ones(corpus.RUNS_N, dtype=bool), CASES["window_runs"].pairs())
    for start, length in corpus.RUNS:
        assert comp[start] == list(range(start, start + length))
    assert sorted((length, start % corpus.CCW_BODIES) for start, length in corpus.RUNS) == [(255, 0), (255, 1), (256, 0), (256, 1), (257, 0), (257, 1)]
    pairs = CASES["window_runs"].pairs()
    assert all(a == b + 1 for a, b in pairs) and pairs[0][0] == 254      # listed from the top down
    awake = set(comp[corpus.RUNS[corpus.RUN_AWAKE][0]])
    slept, state, _ = runs["window_runs"]
    assert set(slept[2]) == set(range(corpus.RUNS_N)) - awake and not state["asleep"][sorted(awake)].any()
    for neighbour in (corpus.RUN_AWAKE - 1, corpus.RUN_AWAKE + 1):
        assert state["asleep"][comp[corpus.RUNS[neighbour][0]]].all()
    # every_kind: one unit of each kind in the chain, the two bodies tied to the world on their own
    case = CASES["every_kind"]
    lists = case.lists()
    chain = [(int(u["body1"][k]), int(u["body2"][k])) for u in lists for k in range(len(u)) if u["body2"][k] >= 0]
    assert sorted(chain) == [(0, 1), (1, 2), (2, 3), (3, 4)] and all((u["body2"] >= 0).sum() == 1 for u in lists)
    assert sorted(int(u["body1"][k]) for u in lists for k in range(len(u)) if u["body2"][k] < 0) == [5, 6]
    assert corpus.components(7, np.ones(7, dtype=bool), case.pairs()) == {0: [0, 1, 2, 3, 4], 5: [5], 6: [6]}
    assert runs["every_kind"][0][2] == [0, 1, 2, 3, 4, 6] and not runs["every_kind"][1]["asleep"][5]


def test_interleaved_pairs_meets_its_wave_premise(runs):
    slept, state, _ = runs["interleaved_pairs"]
    assert [len(x) for x in slept[:6]] == [0, 0, 256, 256, 256, 256]
    block, roots, steps = corpus.wave_premise(slept)
    assert block is not None and len(roots) == corpus.WAVE > corpus.SLEEP_WAVE_ROOTS and len(steps) >= 3
    # every aligned wave holds 64 components, each of which lies in two workgroups
    for block in range(0, corpus.PAIRS_N, corpus.WAVE):
        assert len({b % 512 for b in range(block, block + corpus.WAVE)}) == corpus.WAVE
    assert all(a // 256 != b // 256 for a, b in CASES["interleaved_pairs"].pairs())
    # in the upper half now the lane's own timer decides, now the partner's
    late = {b >= 512 for bodies in CASES["interleaved_pairs"].calms.values() for b in bodies}
    assert late == {True, False}


# ---- the tie, the zeros and the denormals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 7])
def test_the_tie(k):
    t = ksum(k)
    assert t < after(t) <= ksum(k + 1) and ksum(k - 1) < t
    case = corpus.permuted_path(k)
    everybody = list(range(corpus.PATH_N))
    slept, _ = corpus.simulate(case, t, k + 1)
    assert slept == [[]] * (k - 1) + [everybody, []]                       # min timer == time_to_sleep: asleep
    slept, _ = corpus.simulate(case, after(t), k + 1)
    assert slept == [[]] * k + [everybody]                                 # one ulp more: a step later


def test_the_squares_of_the_zeros_case():
    with np.errstate(under="ignore"):
        big, small = F(1e-20) * F(1e-20), F(1e-23) * F(1e-23)
    tiny = np.finfo(np.float32).tiny
    assert 0 < big < tiny                                                  # a float32 denormal: above 0
    assert small == 0 and not np.signbit(small)                            # underflows to +0
    assert F(-0.0) * F(-0.0) == 0 and not np.signbit(F(-0.0) * F(-0.0))
    v = CASES["zeros"].velocities()
    assert v.view(np.uint32)[0].tolist() == [0x80000000] * 3
    calm = CASES["zeros"].calm_from()
    assert [b for b in range(7) if calm[b] == 0] == corpus.ZEROS_CALM and [b for b in range(7) if calm[b] is None] == corpus.ZEROS_NOT


def test_zeros_on_the_spec(runs):
    slept, state, _ = runs["zeros"]
    assert slept[2] == corpus.ZEROS_CALM and not state["asleep"][corpus.ZEROS_NOT].any() and not state["timer"][corpus.ZEROS_NOT].any()


def test_a_negative_zero_survives_a_step_only_under_an_acceleration_that_underflows(oracle):
    """why zeros() gives body 0 the acceleration ZEROS_KEEP: v + (+0) dt is +0 for v = -0; a = +0 + ZEROS_KEEP, as add_accelerations
    adds it, times dt underflows to -0, and (-0) + (-0) is -0"""
    w = oracle.OracleWorld(gravity=0.0)
    w.add_scene(CASES["zeros"].scene())
    b = w.bodies()
    assert b["inv_mass"][0] == 0 and b["inv_inertia"][0] > 0
    for name in ("velocity", "acceleration"):
        for axis in "xy":
            b[name][axis][:2] = -0.0
    b["angular_velocity"][:2] = -0.0
    keep = F(F(0) + corpus.ZEROS_KEEP)
    assert keep < 0 and F(keep * F(DT)) == 0 and np.signbit(F(keep * F(DT)))
    b["acceleration"]["x"][0] = b["acceleration"]["y"][0] = b["angular_acceleration"][0] = keep
    b["acceleration"]["x"][1] = b["acceleration"]["y"][1] = b["angular_acceleration"][1] = F(F(0) + F(-0.0))      # what an added -0 leaves: +0
    w.update(DT, oracle.SOLVE_SCALAR, oracle.ISLAND_SINGLE, 15, 15)
    b = w.bodies()
    got = lambda i: np.array([b["velocity"]["x"][i], b["velocity"]["y"][i], b["angular_velocity"][i]], dtype=np.float32).view(np.uint32).tolist()
    assert got(0) == [0x80000000] * 3 and got(1) == [0, 0, 0]


# ---- the edges exert nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n].pairs()])
def test_the_unit_pass_leaves_every_byte(name, oracle):
    case = CASES[name]
    w = oracle.OracleWorld(gravity=0.0)
    w.add_scene(case.scene())
    bodies = w.bodies().copy()
    v = case.velocities()
    bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"] = v[:, 0], v[:, 1], v[:, 2]
    lists = case.lists()
    before = bodies.tobytes(), [u.tobytes() for u in lists]
    unit_spec.solve_units(bodies, lists, range(sum(len(u) for u in lists)), DT)
    assert bodies.tobytes() == before[0], "a unit of %s moved a body" % name
    assert [u.tobytes() for u in lists] == before[1], "a unit of %s stored an impulse" % name


# ---- the wake by list on the spec ---------------------------------------------------------------------------------------------------------
def test_the_wake_by_list_wakes_breadth_first_components(runs):
    none = np.zeros(0, dtype=manifold_dtype)
    # permuted_path asleep: one named body wakes all 1500
    state = runs["permuted_path"][1].copy()
    assert state["asleep"].all()
    assert sleep_spec.wake_components(state, [777], none, CASES["permuted_path"].pairs()) == list(range(corpus.PATH_N))
    # interleaved_pairs asleep: one body wakes its pair; two of one pair, an awake body and the static one wake that pair
    case = CASES["interleaved_pairs"]
    state = runs["interleaved_pairs"][1].copy()
    assert state["asleep"][:corpus.PAIRS_N].all() and not state["asleep"][corpus.PAIRS_STATIC]
    assert sleep_spec.wake_components(state, [700], none, case.pairs()) == [188, 700]
    assert sleep_spec.wake_components(state, [5, 517, 188, corpus.PAIRS_STATIC], none, case.pairs()) == [5, 517]
    # window_runs: the middle of a sleeping chain wakes that chain only
    start, length = corpus.RUNS[corpus.RUN_CUT]
    state = runs["window_runs"][1].copy()
    assert sleep_spec.wake_components(state, [start + length // 2], none, CASES["window_runs"].pairs()) == list(range(start, start + length))


# ---- Part B -----------------------------------------------------------------------------------------------------------------------------
def test_struck_on_the_oracle(oracle):
    """The oracle carries all of it: a platform's velocity is written into its record.  The column on the platform sleeps at step 2
    with a manifold between its lowest box and the platform; an untouched platform wakes nobody; a velocity, an angular word alone
    and a denormal each wake exactly the column on their platform at the end of the next step.  A -0.0 does not outlive the step
    (sleep_corpus.STRUCK) and wakes nobody."""
    w = oracle.OracleWorld(gravity=corpus.G)
    w.add_scene(corpus.platforms())
    params = sleep_spec.Params(*corpus.STRUCK["params"])
    state = sleep_spec.new_state(12)
    strikes = {s: (p, v, hits) for s, p, v, hits in corpus.STRUCK["strikes"]}
    for step in range(9):
        if step in strikes:
            p, v, hits = strikes[step]
            b = w.bodies()
            b["velocity"]["x"][p], b["velocity"]["y"][p], b["angular_velocity"][p] = v
        w.update(DT, oracle.SOLVE_SCALAR, oracle.ISLAND_SINGLE, 15, 15)
        bodies, manifolds = w.bodies(), w.manifolds()
        was_asleep = state["asleep"].copy()
        slept, woken = sleep_spec.decide_records(state, bodies, manifolds, None, None, params, DT)
        sleep_oracle.apply_to_view(bodies, state, slept, woken)
        if step == corpus.STRUCK["sleep_step"]:
            assert slept == corpus.column(0) + corpus.column(1) + corpus.column(2)
        if step >= corpus.STRUCK["sleep_step"]:
            for c in range(3):
                low, plat = corpus.column(c)[0], corpus.PLATFORMS[c]
                assert any(m["point_count"] > 0 and {int(m["body1"]), int(m["body2"])} == {low, plat} for m in manifolds), \
                    "no manifold with points between sleeper %d and platform %d after step %d" % (low, plat, step)
        if step == corpus.STRUCK["sleep_step"] + 1:
            assert (slept, woken) == ([], []), "an untouched platform woke somebody"
        if step in strikes:
            p, v, hits = strikes[step]
            c = corpus.PLATFORMS.index(p)
            assert was_asleep[corpus.column(c)].all()
            words = np.array([bodies["velocity"]["x"][p], bodies["velocity"]["y"][p], bodies["angular_velocity"][p]], dtype=np.float32).view(np.uint32)
            given = np.array(v, dtype=np.float32).view(np.uint32)
            assert given.any()
            if hits:
                assert words.tolist() == given.tolist(), "the step changed the platform's velocity words"
                assert woken == corpus.column(c), "step %d: platform %d with velocity %s woke %s" % (step, p, v, woken)
            else:
                assert not words.any() and woken == [], "the -0.0 outlived the step"
    given = [np.array(v, dtype=np.float32).view(np.uint32).tolist() for _, _, v, _ in corpus.STRUCK["strikes"]]
    assert [0x80000000, 0, 0] in given and [0, 0, np.array(1e-3, dtype=np.float32).view(np.uint32)] in given
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny


def test_broken_this_step_discriminates():
    """The oracle carries no units beside contacts, so the scene itself runs on the device only, where the test asserts on world B that
    the pin broke in the deciding step and that the two decisions differ.  Here, on the state the case is built to reach - box a calm
    for two passes, box b turning above the angular tolerance - the spec with the broken pin listed lets nobody sleep and without it
    puts a to sleep; and break_spec breaks a pin that carries b's weight under the case's limit."""
    a, b = corpus.BROKEN["a"], corpus.BROKEN["b"]
    params = sleep_spec.Params(*corpus.BROKEN["params"])
    masses = np.array([[0, 0], [1, 1], [1, 1]], dtype=np.float32)
    v = np.zeros((3, 3), dtype=np.float32)
    v[b] = corpus.BROKEN["spin"]
    none = np.zeros(0, dtype=manifold_dtype)

    def decide(units):
        state = sleep_spec.new_state(3)
        state["timer"][a] = ksum(corpus.BROKEN["break_step"])
        got = sleep_spec.decide(state, masses[:, 0], masses[:, 1], v[:, 0], v[:, 1], v[:, 2], none, units, None, params, DT)
        return got, state

    (slept, woken), state = decide(sleep_spec.unit_pairs([corpus.broken_pins()]))
    assert (slept, woken) == ([], []) and state["timer"][a] == params.time_to_sleep and state["timer"][b] == 0
    (slept, woken), _ = decide([])
    assert slept == [a]
    pins = corpus.broken_pins()
    pins["impulse"][0] = (0.0, 1.6e-4 * -corpus.G * DT)      # what holds the 4 x 4 box b (AddBody's mass: 1e-5 x 4 x 4) against gravity for one step
    events = break_spec.breaks([pins], [np.array([corpus.BROKEN["limit"]], dtype=np.float32)], DT)
    assert len(events) == 1 and (events[0]["body1"], events[0]["body2"]) == (a, b)


def test_the_scenes_of_part_b_are_what_their_cases_say():
    """sensor and round: the oracle carries neither flags nor shapes, so their premises are asserted on world B in the device tests;
    here only the geometry the cases rely on"""
    sc = corpus.sensor_scene()
    s, top = corpus.SENSOR_BODY, corpus.SENSOR_COLUMN[-1]
    assert sc["pinned"][s] and not sc["static"][s]
    assert abs(sc["px"][s] - sc["px"][top]) < sc["sx"][s] + sc["sx"][top] and abs(sc["py"][s] - sc["py"][top]) < sc["sy"][s] + sc["sy"][top]   # overlaps the top box
    below = corpus.SENSOR_COLUMN[-2]
    assert sc["py"][s] - np.hypot(sc["sx"][s], sc["sy"][s]) > sc["py"][below] + sc["sy"][below]      # and, however it turns, no other
    sc = corpus.round_scene()
    bodies, radii = corpus.ROUND["circles"]
    notch, roller = bodies
    assert [float(sc["sx"][b]) for b in bodies] == radii
    # the notch circle starts just above the two corners it comes to rest on, the roller on the ground
    for box in (1, 2):
        corner = (sc["px"][box] - np.sign(sc["px"][box]) * sc["sx"][box], sc["py"][box] + sc["sy"][box])
        d = np.hypot(corner[0] - sc["px"][notch], corner[1] - sc["py"][notch])
        assert radii[0] < d < radii[0] + 0.1
    assert sc["py"][roller] - radii[1] == sc["py"][0] + sc["sy"][0]
    vx, _, w = corpus.ROUND["roll"]
    lin, ang, _ = corpus.ROUND["params"]
    assert abs(vx) > lin and abs(w) > ang
    sc = corpus.broken_scene()
    a, b = corpus.BROKEN["a"], corpus.BROKEN["b"]
    pin = corpus.broken_pins()[0]
    assert (sc["px"][a] + pin["anchor1"][0], sc["py"][a] + pin["anchor1"][1]) == (sc["px"][b], sc["py"][b]) and tuple(pin["anchor2"]) == (0.0, 0.0)
    assert sc["py"][b] - np.hypot(sc["sx"][b], sc["sy"][b]) > sc["py"][0] + sc["sy"][0]               # b hangs clear of the ground
    assert sc["px"][b] - np.hypot(sc["sx"][b], sc["sy"][b]) > sc["px"][a] + sc["sx"][a]               # and of a
    assert abs(corpus.BROKEN["spin"][2]) > corpus.BROKEN["params"][1]
