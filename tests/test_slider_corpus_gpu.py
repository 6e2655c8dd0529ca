"""The slider corpus on the device (tests/slider_corpus.py): every case, none left out, through k_solve_pins plain and tethered to a pin,
a link and an angle (the four kinds in one class sequence), and tethered a second time under PHX_PIN_GROUP_PINS=1 through the trailing
group's kernels (k_pin_prestep / k_pin_class); the lockstep of tests/unit_lockstep.py, byte for byte against the spec
(tests/slider_spec.py).  The two cases whose bodies are all static have no component to exceed the cap and run on the LDS path only."""
import pytest

import phyx_amd
import slider_corpus
import unit_lockstep as ul
from unit_spec import SLIDER

pytestmark = pytest.mark.gpu

NO_COMPONENT = ("static_static", "stored_impulses_on_inactive")
RUNS = ([(n, "plain") for n in slider_corpus.NAMES] + [(n, "tethered") for n in slider_corpus.NAMES]
        + [(n, "cap1") for n in slider_corpus.NAMES if n not in NO_COMPONENT])


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_case_on_the_device(oracle, built_lib, monkeypatch, name, path):
    m = slider_corpus.build(name, tether=(path != "plain"))
    if path == "cap1":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "1")
    pw, ow = m.device_world(phyx_amd), m.oracle_world(oracle)
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    units, cfg = ul.lists(pins=m.pins, links=m.links, angles=m.angles, sliders=m.sliders), ul.cfg()
    sched = pw.pin_schedule()
    if path == "cap1":
        assert sched["lds_groups"] == 0 and len(sched["group_offsets"]) == 2, "the whole case in the trailing group"
    elif name not in NO_COMPONENT:
        assert sched["lds_groups"] >= 1
    for s in range(m.steps):
        _, work = ul.step(oracle, pw, ow, cfg, units)
        assert pw.counts()[1] == 0, "bodies touch at step %d" % s
        if s == 0:
            assert [slider_corpus.state_of(w) for w in work[SLIDER]] == m.expect_sliders
        ul.check(pw, ow, units, s)
