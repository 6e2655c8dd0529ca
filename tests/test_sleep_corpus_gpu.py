"""The sleep corpus (tests/sleep_corpus.py) on the device, by twins (tests/sleep_lockstep.py): world A sleeps, world B does not and gets
the spec's decisions as edits; every byte of the state, of the unit lists, of the sleep states and the counts is compared after every
step and every call.  There is no tolerance here.  Every premise a case stands on is asserted where it is used, on world B."""
import numpy as np
import pytest

from phyx_amd import api
from unit_lockstep import lists as unit_lists
from sleep_lockstep import Twins
import sleep_corpus as corpus
import sleep_spec
from sleep_corpus import DT, G, ksum, after

pytestmark = pytest.mark.gpu

NEG0_WORD = 0x80000000


# ---- the means ----------------------------------------------------------------------------------------------------------------------------
def graph_twins(case, time_to_sleep=None):
    t = Twins(case.scene(), (0.0, 0.0, ksum(case.k) if time_to_sleep is None else time_to_sleep), lists=case.lists(), gravity=0.0, prepare=case.prepare)
    assert t.a.counts()[1] == 0, "a graph case has no manifolds"
    return t


def call(t, name, named, *args, wakes=()):
    """a call that names the bodies `named`, on both twins: their sleeping components wake first (`wakes`), then it does what it does"""
    getattr(t.a, name)(named, *args)
    assert t.wake_on_b(named) == list(wakes), "%s of %s" % (name, list(named)[:8])
    getattr(t.b, name)(named, *args)
    t.same("after " + name)


def velocity_words(w, body):
    b = w.body_states([body])
    return np.array([b["velocity"]["x"][0], b["velocity"]["y"][0], b["angular_velocity"][0]], dtype=np.float32).view(np.uint32).tolist()


def words(v):
    return np.array(v, dtype=np.float32).view(np.uint32).tolist()


def run_graph(case, steps, time_to_sleep=None, before=None, after_step=None, bookkeeping=True):
    """the case's twins through `steps` steps; after the first step in which something fell asleep a body-naming call comes before
    anything else, and the pin schedules (the static set is part of them) are compared there and after one more step"""
    t = graph_twins(case, time_to_sleep)
    compare = -1
    for s in range(steps):
        if s in case.calms:
            call(t, "set_velocities", case.calms[s], np.zeros((len(case.calms[s]), 3), dtype=np.float32))
        if before:
            before(t, s)
        t.step(s)
        if after_step:
            after_step(t, s)
        if bookkeeping and case.pairs() and t.slept[-1] and compare < 0:
            spinners = [b for b, first in enumerate(case.calm_from()) if first is None]
            if spinners:                                                    # (awake: the call wakes nobody and changes nothing)
                call(t, "set_velocities", spinners, case.velocities()[spinners])
            compare = s + 1
            t.same_schedules("after step %d, in which %d bodies fell asleep" % (s, len(t.slept[-1])))
        elif s == compare:
            t.same_schedules("one step after the first sleep")
    assert not any(t.woken), "nothing wakes in a graph case"
    return t


def has_points(manifolds, a, b):
    return any(m["point_count"] > 0 and {int(m["body1"]), int(m["body2"])} == {a, b} for m in manifolds)


# ---- Part A: the graph cases --------------------------------------------------------------------------------------------------------------
GRAPHS = {c.name: c for c in corpus.graph_cases()}


@pytest.mark.parametrize("name", ["permuted_path", "cut_path", "star_high", "star_low", "window_runs", "every_kind"])
def test_graph_case(name):
    """labels on hard graphs: the component under its smallest body, whatever order the links, the windows and the workgroups see it in;
    who sleeps in which step, and who never does, is sleep_corpus' breadth-first search and arithmetic (checked against the spec on the
    CPU), the twins hold the device to the spec"""
    case = GRAPHS[name]
    steps = max(s for s in case.sleep_steps().values() if s is not None) + 3
    t = run_graph(case, steps)
    assert t.slept == case.expected_slept(steps)
    assert any(t.slept)
    asleep, slept, woken = t.a.sleep_counts()
    assert (asleep, slept, woken) == (sum(map(len, t.slept)), sum(map(len, t.slept)), 0)


def test_interleaved_pairs_and_its_wake_by_list():
    """many roots in one wave: 64 components per aligned wave, falling asleep in four different steps, the deciding timer now the
    lane's own and now its partner's in another workgroup; then the wake by list on pairs"""
    case = GRAPHS["interleaved_pairs"]
    steps = 7
    t = run_graph(case, steps)
    assert t.slept == case.expected_slept(steps)
    block, roots, when = corpus.wave_premise(t.slept)
    assert block is not None and len(roots) > corpus.SLEEP_WAVE_ROOTS and len(when) >= 3, \
        "no aligned block of 64 bodies holds more than %d components that fell asleep in three different steps: %s" % (corpus.SLEEP_WAVE_ROOTS, (block, len(roots), when))
    assert t.asleep() == list(range(corpus.PAIRS_N))
    call(t, "wake_bodies", [700], wakes=[188, 700])                        # one body: its pair only
    call(t, "wake_bodies", [5, 517, 188, corpus.PAIRS_STATIC], wakes=[5, 517])      # twice one component, an awake body, the static one
    assert t.asleep() == [b for b in range(corpus.PAIRS_N) if b not in (5, 188, 517, 700)]
    for s in range(3):
        t.step(100 + s)
    assert t.slept[-1] == [5, 188, 517, 700]                               # three calm passes later they sleep again


@pytest.mark.parametrize("k", [3, 7])
def test_the_tie(k):
    """min timer >= time_to_sleep, with equality: T is the float32 sum of k time steps as the timer adds them; one ulp more costs a step"""
    case = corpus.permuted_path(k)
    everybody = list(range(corpus.PATH_N))
    t = run_graph(case, k + 1, ksum(k), bookkeeping=False)
    assert t.slept == [[]] * (k - 1) + [everybody, []]
    t = run_graph(case, k + 1, after(ksum(k)), bookkeeping=False)
    assert t.slept == [[]] * k + [everybody]


def test_zeros():
    """tolerance 0: -0.0 is calm, a velocity whose square is a float32 denormal is not, one whose square underflows to +0 is; the same
    for the angular word.  The premises, on world B after the step: the -0.0 words and the tiny velocities are still there."""
    case = GRAPHS["zeros"]
    keep = np.full((1, 3), corpus.ZEROS_KEEP, dtype=np.float32)      # (its product with dt underflows to -0: sleep_corpus.zeros)

    def before(t, s):
        if not t.state["asleep"][0]:
            call(t, "add_accelerations", [0], keep)

    def after_step(t, s):
        for b, v in corpus.ZEROS.items():
            if not t.state["asleep"][b]:
                assert velocity_words(t.b, b) == words(v), "step %d changed the velocity words of body %d: the case's premise" % (s, b)

    t = run_graph(case, 6, before=before, after_step=after_step)
    assert words(corpus.ZEROS[0]) == [NEG0_WORD] * 3
    assert t.slept == [[], [], corpus.ZEROS_CALM, [], [], []]
    assert not t.state["asleep"][corpus.ZEROS_NOT].any() and not t.state["timer"][corpus.ZEROS_NOT].any()
    assert not t.a.sleep_states()["timer"][corpus.ZEROS_NOT].any()


def test_wake_by_list_on_the_path():
    case = GRAPHS["permuted_path"]
    t = run_graph(case, 3, bookkeeping=False)
    everybody = list(range(corpus.PATH_N))
    assert t.asleep() == everybody
    call(t, "wake_bodies", [777], wakes=everybody)
    assert t.a.sleep_counts() == (0, corpus.PATH_N, corpus.PATH_N)
    for s in range(3):
        t.step(100 + s)
    assert t.asleep() == everybody


def test_removing_the_middle_of_a_sleeping_chain():
    """remove_bodies names the body: its chain wakes, and only it; the world goes on with the remapped lists, the chain in two parts"""
    case = GRAPHS["window_runs"]
    t = run_graph(case, 3, bookkeeping=False)
    start, length = corpus.RUNS[corpus.RUN_CUT]
    gone, run = start + length // 2, list(range(start, start + length))
    asleep = t.asleep()
    assert set(run) <= set(asleep)
    assert t.wake_on_b([gone]) == run
    remap = t.a.remove_bodies([gone])
    assert remap.tobytes() == t.b.remove_bodies([gone]).tobytes()
    t.state = t.state[remap >= 0].copy()
    t.same("after the removal")
    assert t.asleep() == [int(remap[b]) for b in asleep if b not in run]
    for s in range(3):
        t.step(100 + s)
    assert t.slept[-1] == [int(remap[b]) for b in run if b != gone]        # two chains now, calm for three passes
    assert t.a.link_count() == len(case.ropes) - 2


# ---- Part B: the clauses that need a real step ------------------------------------------------------------------------------------------------
def test_struck():
    """a sleeper that shares a manifold with points with a body outside the mobile set whose velocity has a nonzero word wakes at the
    end of that step, and only its component: a velocity, an angular word alone, a denormal.  A -0.0 does not outlive the step on a
    body that has a contact (sleep_corpus.STRUCK): asserted on world B, and then it strikes nobody."""
    t = Twins(corpus.platforms(), corpus.STRUCK["params"], gravity=G)
    strikes = {s: (p, v, hits) for s, p, v, hits in corpus.STRUCK["strikes"]}
    columns = corpus.column(0) + corpus.column(1) + corpus.column(2)
    for s in range(9):
        if s in strikes:
            p, v, hits = strikes[s]
            assert set(corpus.column(corpus.PLATFORMS.index(p))) <= set(t.asleep())
            call(t, "set_velocities", [p], np.array([v], dtype=np.float32))
            assert velocity_words(t.b, p) == words(v)
        t.step(s)
        if s == corpus.STRUCK["sleep_step"]:
            assert t.slept[-1] == columns
        if s >= corpus.STRUCK["sleep_step"]:
            manifolds = t.b.manifolds
            for c in range(3):
                low, plat = corpus.column(c)[0], corpus.PLATFORMS[c]
                assert has_points(manifolds, low, plat), "no manifold with points between %d and its platform %d after step %d" % (low, plat, s)
        if s == corpus.STRUCK["sleep_step"] + 1:
            assert (t.slept[-1], t.woken[-1]) == ([], []), "an untouched platform woke somebody"
        if s in strikes:
            p, v, hits = strikes[s]
            if hits:
                assert velocity_words(t.b, p) == words(v), "the step changed the platform's velocity words"
                assert t.woken[-1] == corpus.column(corpus.PLATFORMS.index(p)), "step %d: platform %d, velocity %s" % (s, p, v)
            else:
                assert velocity_words(t.b, p) == [0, 0, 0], "the -0.0 outlived the step: sleep_corpus.STRUCK says it cannot"
                assert t.woken[-1] == []


def test_sensor():
    """a sensor's manifolds are no edge: a sensor that never calms down lies across the top of a calm column, with points; the column
    falls asleep without it and stays asleep under it; with the flag cleared the next pass joins them and the column wakes"""
    s_body, col = corpus.SENSOR_BODY, corpus.SENSOR_COLUMN

    def prepare(w):
        w.set_body_flags([s_body], [api.BODY_SENSOR])
        w.set_velocities([s_body], np.array([corpus.SENSOR_SPIN], dtype=np.float32))

    t = Twins(corpus.sensor_scene(), corpus.SENSOR["params"], gravity=G, prepare=prepare)
    t.flags = True
    for s in range(corpus.SENSOR["clear_before"]):
        t.step(s)
        assert has_points(t.b.manifolds, s_body, col[-1]), "no manifold with points between the sensor and the top box after step %d" % s
        assert t.state["timer"][s_body] == 0 and not t.state["asleep"][s_body], "the sensor calmed down"
        assert t.asleep() == (col if s >= corpus.SENSOR["sleep_step"] else [])
        assert t.woken[-1] == []
    assert t.slept[corpus.SENSOR["sleep_step"]] == col
    call(t, "set_body_flags", [s_body], [0])
    assert t.asleep() == col
    t.step(corpus.SENSOR["clear_before"])
    assert has_points(t.b.manifolds, s_body, col[-1])
    assert t.woken[-1] == col, "without the flag the awake box across its top wakes the column"


def test_broken_this_step():
    """a unit that broke in this step is still an edge in it: in the pass of the step in which the pin breaks, box a's timer reaches
    time_to_sleep and box b, turning on the pin, has timer 0 - with the pin as an edge nobody sleeps, without it a would"""
    a, b, step = corpus.BROKEN["a"], corpus.BROKEN["b"], corpus.BROKEN["break_step"]
    t = Twins(corpus.broken_scene(), corpus.BROKEN["params"], lists=unit_lists(pins=corpus.broken_pins()), gravity=G,
              prepare=lambda w: w.set_velocities([b], np.array([corpus.BROKEN["spin"]], dtype=np.float32)))
    for s in range(step):
        t.step(s)
        assert len(t.a.break_events()) == len(t.b.break_events()) == 0
    t.a.set_break_limits("pin", [0], [corpus.BROKEN["limit"]])
    assert t.wake_on_b([a, b]) == []
    t.b.set_break_limits("pin", [0], [corpus.BROKEN["limit"]])
    t.same("after set_break_limits")
    before = t.state.copy()
    t.step(step)
    events = t.a.break_events()
    assert events.tobytes() == t.b.break_events().tobytes()
    assert len(events) == 1 and (events[0]["kind"], events[0]["index"], events[0]["body1"], events[0]["body2"]) == (0, 0, a, b), \
        "the pin did not break in step %d: %s" % (step, events)
    assert t.a.pin_count() == t.b.pin_count() == 0
    # the discriminating pair of decisions, on the step's own result (nobody fell asleep, so B's records are the step's)
    assert (t.slept[-1], t.woken[-1]) == ([], [])
    params = sleep_spec.Params(*corpus.BROKEN["params"])
    with_pin, without = before.copy(), before.copy()
    assert sleep_spec.decide_records(with_pin, t.b.bodies, t.b.manifolds, [corpus.broken_pins()], None, params, DT) == ([], [])
    assert sleep_spec.decide_records(without, t.b.bodies, t.b.manifolds, None, None, params, DT) == ([a], []), "the case does not discriminate"
    assert with_pin["timer"][a] == params.time_to_sleep and with_pin["timer"][b] == 0
    t.same_schedules("after the step of the break")
    t.step(step + 1)
    assert t.slept[-1] == [a], "in the step after, the edge is gone"
    t.same_schedules("one step after the break")
    assert len(t.a.break_events()) == len(t.b.break_events()) == 0


def test_round():
    """round bodies: a circle at rest in the notch between two boxes and a circle rolling on the ground; the pile sleeps, the roller does
    not while it rolls; a circle dropped on the pile wakes the component it hits.  (The oracle carries no shapes: every premise is
    asserted here on world B.)"""
    pile, roller = corpus.ROUND["pile"], corpus.ROUND["roller"]
    bodies, radii = corpus.ROUND["circles"]
    lin = corpus.ROUND["params"][0]

    def prepare(w):
        w.set_shapes(bodies, api.SHAPE_CIRCLE, radii)
        w.set_inverse_masses(bodies, api.circle_inverse_masses(radii))
        w.set_velocities([roller], np.array([corpus.ROUND["roll"]], dtype=np.float32))

    t = Twins(corpus.round_scene(), corpus.ROUND["params"], gravity=G, prepare=prepare)
    assert t.a.shapes()["kind"].tolist() == [0, 0, 0, 1, 1]
    for s in range(40):
        t.step(s)
        if t.slept[-1]:
            break
    assert t.slept[-1] == pile, "the pile did not fall asleep as one within 40 steps"
    manifolds = t.b.manifolds
    assert has_points(manifolds, 1, 3) and has_points(manifolds, 2, 3), "the circle does not rest on both boxes of the notch"
    v = t.b.body_states([roller])["velocity"]
    assert np.hypot(float(v["x"][0]), float(v["y"][0])) > lin and not t.state["asleep"][roller], "the roller does not roll any more"
    first = t.a.add_circles(np.array([corpus.ROUND["drop"]], dtype=np.float32))
    assert first == t.b.add_circles(np.array([corpus.ROUND["drop"]], dtype=np.float32)) == 5
    t.state = sleep_spec.grown(t.state, 6)
    t.same("after the spawn")
    call(t, "set_velocities", [first], np.array([corpus.ROUND["drop_velocity"]], dtype=np.float32))
    for s in range(20):
        t.step(100 + s)
        if t.woken[-1]:
            break
    assert t.woken[-1] == pile, "the dropped circle should wake the pile it lands on"
    assert has_points(t.b.manifolds, first, 3)
    for s in range(3):
        t.step(200 + s)
