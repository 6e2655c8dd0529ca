"""The link corpus on the device (tests/link_corpus.py): every case through k_solve_pins and, tethered, a second time under
PHX_PIN_GROUP_PINS=1 through the trailing group's kernels (k_pin_prestep / k_pin_class); the lockstep of tests/unit_lockstep.py, byte
for byte against the spec (tests/link_spec.py) on velocities and impulses.  The two cases that overflow compare NaN as NaN: which NaN a
processor makes of inf - inf is its own affair, that it makes one is the spec's."""
import numpy as np
import pytest

import phyx_amd
import link_corpus
import unit_lockstep as ul
from unit_spec import LINK

pytestmark = pytest.mark.gpu

RUNS = [(n, "lds") for n in link_corpus.NAMES] + [(n, "cap1") for n in link_corpus.NAMES if n not in ("static_static", "static_world")]


def _floats(a):
    return np.frombuffer(a.tobytes(), dtype=np.float32)


def _same_numbers(a, b):
    """bit for bit, but for NaNs, which only have to sit in the same places"""
    x, y = _floats(a), _floats(b)
    nan = np.isnan(x)
    return np.array_equal(nan, np.isnan(y)) and x[~nan].tobytes() == y[~nan].tobytes()


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_case_on_the_device(oracle, built_lib, monkeypatch, name, path):
    m = link_corpus.build(name, tether=(path == "cap1"))
    if path == "cap1":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "1")
    pw, ow = m.device_world(phyx_amd), m.oracle_world(oracle)
    links, cfg = m.links, ul.cfg()
    units = ul.lists(pins=m.pins, links=links)
    sched = pw.pin_schedule()
    if path == "cap1":
        assert sched["lds_groups"] == 0 and len(sched["group_offsets"]) == 2, "the whole case in the trailing group"
    else:
        assert sched["lds_groups"] >= (1 if "active" in m.expect else 0)
    for s in range(m.steps):
        if s == 1 and m.edit:
            k, anchors = m.edit
            pw.set_link_anchors([k], np.array([anchors], dtype=np.float32))
            links["anchor1"][k], links["anchor2"][k] = anchors[:2], anchors[2:]
        _, work = ul.step(oracle, pw, ow, cfg, units)
        assert pw.counts()[1] == 0, "bodies touch at step %d" % s
        if s == 0:
            assert [link_corpus.state_of(w) for w in work[LINK]] == m.expect
        if s == 1 and m.edit:
            assert not np.isfinite(links["impulse"][m.edit[0]]), "the edit did not overflow the impulse"
            got, want = pw.bodies, ow.bodies()
            for f in ("velocity", "angular_velocity"):
                assert _same_numbers(got[f], want[f]), "%s differ at step %d" % (f, s)
            assert _same_numbers(pw.links()["impulse"], links["impulse"]), "impulses differ at step %d" % s
            assert np.isinf(_floats(got["velocity"])).any() or np.isnan(_floats(got["velocity"])).any()
        else:
            ul.check(pw, ow, units, s)
