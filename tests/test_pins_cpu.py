"""Pins without a GPU (include/phyx_amd.h PINS): the new symbols, the host-only schedule builder on small graphs, and the specification
(tests/pin_spec.py) on its own: it must hold a pendulum and a chain together (tests/test_pin_corpus_cpu.py holds it to an independent
float64 reference)."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import _lib, api
import pin_corpus
import pin_spec
import unit_spec

SYMBOLS = ("phx_world_add_pins", "phx_world_remove_pins", "phx_world_set_pin_anchors", "phx_world_get_pins", "phx_world_pin_count",
           "phx_world_set_pin_iterations", "phx_world_get_pin_iterations", "phx_world_pin_schedule_builds", "phx_world_get_pin_schedule",
           "phx_pin_schedule")


def test_symbols_are_exported_and_bound(built_lib):
    for name in SYMBOLS:
        assert hasattr(built_lib, name), name
        assert name in _lib.declared_symbols(), name
    for method in ("add_pins", "remove_pins", "set_pin_anchors", "pins", "pin_iterations", "pin_schedule", "pin_schedule_builds", "pin_count"):
        assert hasattr(phyx_amd.World, method), method
    assert api.pin_dtype.itemsize == 32


def _chain(first_body, links, hang_from):
    """pins of a chain: body first_body hangs from `hang_from` (-1: the world), each next body from the one before."""
    return [(first_body + k, hang_from if k == 0 else first_body + k - 1) for k in range(links)]


def _graph(name):
    """(body1, body2, is_static, group_pins)"""
    if name == "world_pin":
        return [0], [-1], [0], 256
    if name == "pair":
        return [0], [1], [0, 0], 256
    if name == "chain3":
        p = _chain(0, 3, -1)
        return [a for a, _ in p], [b for _, b in p], [0] * 3, 256
    if name == "chain40_cap16":
        p = _chain(0, 40, -1)
        return [a for a, _ in p], [b for _, b in p], [0] * 40, 16
    if name == "pairs300":
        return list(range(0, 600, 2)), list(range(1, 600, 2)), [0] * 600, 256
    if name == "pendulums50":
        return list(range(1, 51)), [0] * 50, [1] + [0] * 50, 256
    raise KeyError(name)


GRAPHS = ("world_pin", "pair", "chain3", "chain40_cap16", "pairs300", "pendulums50")


@pytest.mark.parametrize("name", GRAPHS)
def test_pin_schedule_on_small_graphs(built_lib, name):
    b1, b2, st, cap = _graph(name)
    s = api.pin_schedule(b1, b2, st, group_pins=cap)
    pin_corpus.check_schedule(b1, b2, st, s, cap, name)          # every pin once, classes and groups body-disjoint, the cap kept
    coff, goff = s["class_offsets"], s["group_offsets"]
    if name == "pendulums50":
        assert len(coff) - 1 == 1, "50 pendulums on one static body need one class"
    if name == "chain40_cap16":
        assert s["lds_groups"] == 0 and len(goff) - 1 == 1, "a chain that exceeds the cap goes to the trailing group"
    if name == "chain3":
        assert len(coff) - 1 == 2 and s["lds_groups"] == 1
    if name == "pairs300":
        # (a group never spans a multiple of 64 components — the builder's binning rule — so 300 one-pin components make 5 groups)
        assert s["lds_groups"] == 5 and len(goff) - 1 == 5 and len(coff) - 1 == 5      # one class each


def test_pin_schedule_refuses_bad_arguments(built_lib):
    with pytest.raises(phyx_amd.PhxError):
        api.pin_schedule([0], [0], [0])
    with pytest.raises(phyx_amd.PhxError):
        api.pin_schedule([0], [2], [0, 0])
    with pytest.raises(phyx_amd.PhxError):
        api.pin_schedule([0], [-1], [0], group_pins=0)
    with pytest.raises(phyx_amd.PhxError):
        api.pin_schedule([0], [-1], [0], group_pins=257)


DT, G, SPACING = 1.0 / 60.0, -200.0, 10.0
# The largest anchor separation |C| any prestep of 300 steps saw, measured with the spec itself (n = 8, gravity -200, dt 1/60, links of
# 8 x 3 spaced 10 apart, released level with the anchor so that they swing through the whole arc):
# pendulum 0.132867, 12-chain 1.82392 (the free end whips through the bottom of the arc) — both under a quarter of the spacing, 2.5.
MEASURED = {"pendulum": 0.132867, "chain12": 1.82392}


@pytest.mark.parametrize("name,links", [("pendulum", 1), ("chain12", 12)])
def test_spec_holds_a_chain_together(name, links):
    rows, pins = pin_spec.chain(links, spacing=SPACING)
    bodies = pin_spec.make_bodies(rows)
    order = np.arange(links)
    worst, lowest = 0.0, 300.0
    for _ in range(300):
        worst = max(worst, unit_spec.worst_c(unit_spec.step_free(bodies, [pins], order, DT, G, iterations=8)[unit_spec.PIN]))
        lowest = min(lowest, float(bodies["pos"]["y"].min()))
    print("largest |C| of %s: %.6g" % (name, worst))
    assert np.isfinite(bodies["pos"]["x"]).all() and np.isfinite(bodies["pos"]["y"]).all()
    assert MEASURED[name] < SPACING / 4, "the spec's parameters are wrong: fix the spec, not the bound"
    assert worst < 2 * MEASURED[name]
    assert lowest < 300.0 - 0.4 * SPACING * links, "the chain never swung down"


def test_an_inactive_pin_changes_nothing():
    bodies = pin_spec.make_bodies([(0.0, 0.0, 5.0, 5.0, True), (30.0, 0.0, 5.0, 5.0, True), (60.0, 0.0, 5.0, 5.0, False)])
    bodies["velocity"]["x"][:] = (1.0, -2.0, 3.0)
    pins = np.zeros(1, dtype=api.pin_dtype)
    pins[0] = (0, 1, (5.0, 0.0), (-5.0, 0.0), (7.0, -7.0))
    before = bodies.copy()
    unit_spec.solve_units(bodies, [pins], [0], DT, 8)
    assert bodies.tobytes() == before.tobytes()
    assert pins["impulse"].tolist() == [[0.0, 0.0]], "an inactive pin reads impulse 0"
