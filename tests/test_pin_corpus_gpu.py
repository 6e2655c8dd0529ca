"""The pin corpus on the device (tests/pin_corpus.py): every motif through k_solve_pins on its own schedule and, where it has more than
one pin, a second time under PHX_PIN_GROUP_PINS=1 through the trailing group's kernels.  Each run is judged twice:
  - the lockstep of tests/unit_lockstep.py, byte for byte against the spec (tests/pin_spec.py), for a few steps;
  - the first step's velocities against the float64 reference (tests/pin_reference.py) run on the oracle's pre_solve output, within
    8 x the reference's own float32-vs-float64 deviation on that motif (no contact forms, so the velocities after Update are the
    pass's output),
and the device's own schedule is held to the host builder's and to the shape the motif claims.  The three reference-free checks of
tests/test_pin_corpus_cpu.py run on device output as well."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import api
import pin_corpus
import pin_reference as ref
import unit_reference
import unit_lockstep as ul
from pin_corpus import CONSERVING, INACTIVE, MARGIN, ONE_PIN, ULP, check_momentum, check_residual, check_the_anchor_is_followed

pytestmark = pytest.mark.gpu

DT = pin_corpus.DT
RUNS = [(n, "lds", i) for n in pin_corpus.NAMES for i in pin_corpus.build(n).iterations] + \
       [(n, "cap1", i) for n in pin_corpus.MULTI for i in pin_corpus.build(n).iterations]


def _worlds(oracle, monkeypatch, m, path, iterations, gravity=None):
    cap = 1 if path == "cap1" else m.cap
    if cap:
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", str(cap))
    pw = m.device_world(phyx_amd, gravity)
    pw.pin_iterations = iterations
    return pw, m.oracle_world(oracle, gravity), cap or 256


def _after_first_step(m, before, pw):
    """`before` (the oracle's pre_solve output) with the device's velocities after the step"""
    after, got = before.copy(), pw.bodies
    assert len(got) == len(before)
    after["velocity"], after["angular_velocity"] = got["velocity"], got["angular_velocity"]
    return after


@pytest.mark.parametrize("name,path,iterations", RUNS, ids=["%s-%s-n%d" % r for r in RUNS])
def test_motif_on_the_device(oracle, built_lib, monkeypatch, name, path, iterations):
    m = pin_corpus.build(name)
    pw, ow, cap = _worlds(oracle, monkeypatch, m, path, iterations)
    b1, b2, st = m.graph()
    sched = pw.pin_schedule()
    host = api.pin_schedule(b1, b2, st, group_pins=cap)
    for key in ("order", "class_offsets", "group_offsets"):
        assert sched[key].tolist() == host[key].tolist(), "the device's schedule is the host builder's: %s" % key
    assert sched["lds_groups"] == host["lds_groups"]
    pin_corpus.check_schedule(b1, b2, st, sched, cap, name)
    if path == "lds":
        assert pin_corpus.shape_of(sched) == m.shape
    elif name in pin_corpus.CONNECTED:
        assert sched["lds_groups"] == 0 and len(sched["group_offsets"]) == 2, "the whole motif in the trailing group"

    # the pass's input at the first step, from a second oracle world
    probe = m.oracle_world(oracle)
    probe.pre_solve(DT)
    before = probe.bodies().copy()
    exact = unit_reference.solve(before, [m.pins], sched["order"], DT, iterations, np.float64)
    single = unit_reference.solve(before, [m.pins], sched["order"], DT, iterations, np.float32)
    noise = max(ref.deviation(single.q, exact.q), ULP)
    impulse_noise = max(ref.deviation(single.pin_impulse, exact.pin_impulse), ULP)

    pins, cfg = m.pins, ul.cfg()
    steps = min(m.steps, 3) if (name == "hub130" and path == "cap1") else m.steps
    for s in range(steps):
        ul.step(oracle, pw, ow, cfg, [pins])
        assert pw.counts()[1] == 0, "bodies touch at step %d" % s
        ul.check(pw, ow, ul.lists(pins=pins), s)
        if s:
            continue
        after = _after_first_step(m, before, pw)
        dev = ref.deviation(ref.velocities(after), exact.q)
        print("%-24s %-4s n=%d noise %.3g device %.3g ratio %.2f%s" % (name, path, iterations, noise, dev, dev / noise, " x" if noise > pin_corpus.EXCLUDE_ABOVE else ""))
        if noise > pin_corpus.EXCLUDE_ABOVE:
            assert name in pin_corpus.MAY_BE_EXCLUDED, "%s is too ill-conditioned for the comparison (%.3g)" % (name, noise)
        else:
            assert dev <= MARGIN * noise
            assert ref.deviation(pw.pins()["impulse"], exact.pin_impulse) <= MARGIN * impulse_noise, "the accumulated impulses"
        if name in ONE_PIN and iterations == 1:
            check_residual(before, after, m.pins[0])
        if name in INACTIVE:
            assert after.tobytes() == before.tobytes(), "an inactive pin changed a velocity"
            assert not pw.pins()["impulse"].any(), "an inactive pin reads impulse 0"
    if name == "kinematic_anchor":
        start = m.oracle_world(oracle)
        check_the_anchor_is_followed(m, start.bodies().copy(), pw.bodies, steps)


MOMENTUM_RUNS = [(n, "lds") for n in CONSERVING] + [(n, "cap1") for n in CONSERVING if n in pin_corpus.MULTI]


@pytest.mark.parametrize("name,path", MOMENTUM_RUNS, ids=["%s-%s" % r for r in MOMENTUM_RUNS])
def test_the_pass_conserves_momentum_on_the_device(oracle, built_lib, monkeypatch, name, path):
    """gravity 0, no static body, no world pin: one step; sum m v and sum (m x cross v - I w) from the device's velocities"""
    m = pin_corpus.build(name)
    pw, ow, _ = _worlds(oracle, monkeypatch, m, path, 8, gravity=0.0)
    before = ow.bodies().copy()
    pw.Update(DT, ul.cfg())
    assert pw.counts()[1] == 0
    after = _after_first_step(m, before, pw)
    assert after["velocity"].tobytes() != before["velocity"].tobytes()
    check_momentum(m, before, after, pw.pins()["impulse"], 8)
