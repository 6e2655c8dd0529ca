"""Links without a GPU (include/phyx_amd.h LINKS): the ABI; the specification (tests/link_spec.py) holding a rod, a rope and a spring
together; the host schedule builder on a concatenated list of units; the corpus' claims (tests/link_corpus.py); and the spec held to the
float64 reference (tests/link_reference.py)."""
import ctypes as C

import numpy as np
import pytest

from phyx_amd import api
import link_corpus
import link_reference as lref
import link_spec
import pin_corpus
import pin_spec
import unit_reference
import unit_spec

F = np.float32
DT = 1.0 / 60.0
G = -200.0
NO_PINS = np.zeros(0, dtype=api.pin_dtype)


# ---- the ABI ----
def test_link_record_is_48_bytes():
    assert api.link_dtype.itemsize == 48
    assert [api.link_dtype.fields[f][1] for f in ("body1", "body2", "anchor1", "anchor2", "min_length", "max_length", "hertz", "damping_ratio",
                                                    "impulse", "reserved")] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 44]


def test_the_library_has_the_calls(built_lib):
    lib = C.CDLL(built_lib) if isinstance(built_lib, str) else built_lib
    for name in ("phx_world_add_links", "phx_world_remove_links", "phx_world_set_link_anchors", "phx_world_set_link_lengths",
                 "phx_world_get_links", "phx_world_link_count"):
        assert hasattr(lib, name), name


# ---- the spec holds things together ----
def _one_body(link, steps, pos, gravity=G):
    """one 2 x 2 box at `pos` on the world link `link`: -> per step (the prestep's record, pos.x, pos.y), and free fall's positions"""
    b = pin_spec.make_bodies([(pos[0], pos[1], 2.0, 2.0, False)])
    free = b.copy()
    links = link_spec.make_links([link])
    none = link_spec.make_links([])
    out, fall = [], []
    for _ in range(steps):
        w = unit_spec.step_free(b, [NO_PINS, links], [0], DT, gravity)[unit_spec.LINK][0]
        unit_spec.step_free(free, [NO_PINS, none], [], DT, gravity)
        out.append((w, b["pos"].copy().tobytes()))
        fall.append(free["pos"].copy().tobytes())
    return out, fall, b


def test_a_rod_holds_its_length():
    """released level, it swings through the bottom; observed: len in [50.0, 50.27] over 600 steps.  The bound is not that figure: a
    body that enters a step on the circle leaves it along the tangent, v dt = sqrt(2 g L) dt = 2.36 at the bottom, and is then
    sqrt(L^2 + 2.36^2) - L = 0.056 off; the bias takes a fifth of the error back per step, so the error settles below 5 x 0.056 = 0.28,
    and twice that is the bound"""
    out, _, b = _one_body((0, -1, (0.0, 0.0), (0.0, 0.0), 50.0, 50.0), 600, (50.0, 0.0))
    lens = np.array([float(w.len) for w, _ in out])
    print("rod: len in [%.6g, %.6g]" % (lens.min(), lens.max()))
    assert all(w.active for w, _ in out)
    drift = np.hypot(np.sqrt(2.0 * -G * 50.0) * DT, 50.0) - 50.0
    assert np.abs(lens - 50.0).max() < 2.0 * 5.0 * drift
    ys = np.array([np.frombuffer(p, dtype=np.float32)[1] for _, p in out])
    assert ys.min() < -49.0, "it never swung through the bottom"


def test_a_rope_is_free_fall_until_it_is_taut():
    """released 20 below the anchor on a rope of 50: 30 of free fall take sqrt(2 x 30 / 200) = 0.548 s = 33 steps"""
    out, fall, _ = _one_body((0, -1, (0.0, 0.0), (0.0, 0.0), 0.0, 50.0), 120, (0.0, -20.0))
    idle = [w.idle for w, _ in out]
    first = idle.index(False)
    print("rope: idle for %d steps, len at the end %.8g" % (first, float(out[-1][0].len)))
    assert 30 <= first <= 36 and all(idle[:first])
    for s in range(first):
        assert out[s][1] == fall[s], "an idle rope changed a bit at step %d" % s
    assert out[first][0].active and float(out[first][0].len) >= 50.0, "it engages the step after it overshoots"
    assert all(w.active for w, _ in out[-60:]), "at rest on the rope it is taut on every step"
    assert abs(float(out[-1][0].len) - 50.0) < 1e-3
    assert all(float(w.lam) <= 0 for w, _ in out), "a rope only pulls"


@pytest.mark.parametrize("zeta", [0.0, 1.0])
def test_a_spring_has_its_period_and_its_damping(zeta):
    """1 Hz, no gravity, released 10 from rest: undamped C changes sign every half period = 30 steps; critically damped never"""
    out, _, _ = _one_body((0, -1, (0.0, 0.0), (0.0, 0.0), 40.0, 40.0, 1.0, zeta), 600, (50.0, 0.0), gravity=0.0)
    c = np.array([float(w.c) for w, _ in out])
    changes = np.flatnonzero(np.sign(c[1:]) != np.sign(c[:-1]))
    print("spring zeta %g: %d sign changes, spacing %s, |C| at the end %.3g" % (zeta, len(changes), sorted(set(np.diff(changes).tolist())), abs(c[-1])))
    if zeta == 0.0:
        assert len(changes) >= 18
        assert (np.abs(np.diff(changes) - 30) <= 1).all()
    else:
        assert len(changes) == 0


# ---- the schedule builder on pins followed by links ----
def test_schedule_of_a_chain_of_pins_plus_links():
    rows, pins = pin_spec.chain(12)
    links = [(k, k - 2) for k in range(2, 12, 3)] + [(11, -1), (5, -1)]              # rods across the chain, two ropes to the world
    b1 = pins["body1"].tolist() + [a for a, _ in links]
    b2 = pins["body2"].tolist() + [b for _, b in links]
    st = [0] * len(rows)
    for cap in (256, 4):
        s = api.pin_schedule(b1, b2, st, group_pins=cap)
        pin_corpus.check_schedule(b1, b2, st, s, cap, "chain + links")      # a permutation of the units; no class shares a dynamic body


# ---- the corpus ----
def _pre_solve_bodies(oracle, m):
    ow = m.oracle_world(oracle)
    ow.pre_solve(DT)
    assert len(ow.manifolds()) == 0, "%s: bodies touch" % m.name
    return ow.bodies().copy()


def _order(m):
    b1, b2, st = m.unit_graph()
    return api.pin_schedule(b1, b2, st)["order"]


@pytest.mark.parametrize("tether", [False, True], ids=["plain", "tethered"])
@pytest.mark.parametrize("name", link_corpus.NAMES)
def test_case_reaches_what_it_claims(built_lib, oracle, name, tether):
    m = link_corpus.build(name, tether)
    bodies = _pre_solve_bodies(oracle, m)
    before = bodies.copy()
    pins, links = m.pins, m.links
    work = unit_spec.solve_units(bodies, [pins, links], _order(m), DT, 8)[unit_spec.LINK]
    assert [link_corpus.state_of(w) for w in work] == m.expect
    for k, w in enumerate(work):
        if not w.active:
            assert links["impulse"][k] == 0, "an inactive or idle link reads impulse 0"
    if not any(w.active for w in work) and not len(pins):
        assert bodies.tobytes() == before.tobytes(), "a world of inactive links changed a velocity"
    elif name not in ("rope_moving_inwards", "at_max"):
        assert bodies.tobytes() != before.tobytes(), "the case does nothing"
    if name in ("at_max", "at_min"):
        assert float(work[0].c) == 0.0 and work[0].active
    if name.startswith("warm_start_of_the_wrong_sign"):
        assert float(m.links["impulse"][0]) * float(links["impulse"][0]) < 0, "the stored impulse's sign survived the clamp"
    if name == "rope_moving_inwards":
        assert work[0].active and links["impulse"][0] == 0 and bodies.tobytes() == before.tobytes()


def test_the_square_root_arguments_sit_on_rounding_boundaries():
    assert len(link_corpus.SQRT_D) >= 16
    for d in link_corpus.SQRT_D:
        assert link_corpus.sqrt_midpoint_distance(d) < 2.0 ** -30, d
    # and numpy's float32 sqrt, the spec's, rounds every one of them correctly
    for d in link_corpus.SQRT_D:
        s = F(F(d[0]) * F(d[0])) + F(F(d[1]) * F(d[1]))
        assert np.sqrt(s) == F(np.sqrt(np.float64(s)))


# ---- the spec against the float64 reference ----
# The largest relative deviation of the accumulated impulses after one pass, spec against reference, measured over the scenes and
# the corpus below: 1.14e-05 (sqrt_22: a rod half a unit off its length of 83, where half an ulp of len, 3.8e-6, is 7.6e-6 of C).
# Times 4, the headroom for another libm under numpy.
MEASURED = 1.14e-05
BOUND = 4.0 * MEASURED


def _scenes():
    """the three scenes above at their first engaged step, as (bodies, links)"""
    for link, pos, steps, gravity in (((0, -1, (0.0, 0.0), (0.0, 0.0), 50.0, 50.0), (50.0, 0.0), 40, G),
                                      ((0, -1, (0.0, 0.0), (0.0, 0.0), 0.0, 50.0), (0.0, -20.0), 40, G),
                                      ((0, -1, (0.0, 0.0), (0.0, 0.0), 40.0, 40.0, 1.0, 0.0), (50.0, 0.0), 10, 0.0),
                                      ((0, -1, (0.0, 0.0), (0.0, 0.0), 40.0, 40.0, 1.0, 1.0), (50.0, 0.0), 10, 0.0)):
        b = pin_spec.make_bodies([(pos[0], pos[1], 2.0, 2.0, False)])
        links = link_spec.make_links([link])
        for _ in range(steps):
            unit_spec.step_free(b, [NO_PINS, links], [0], DT, gravity)
        b["velocity"]["y"][0] = F(b["velocity"]["y"][0]) + F(gravity) * F(DT)
        yield b, links


def _compare(bodies, lists, order, what):
    exact = unit_reference.solve(bodies, lists, order, DT, 8)
    own = [units.copy() for units in lists]
    work = unit_spec.solve_units(bodies.copy(), own, order, DT, 8)[unit_spec.LINK]
    assert [w.active for w in work] == exact.link_active.tolist(), "%s: the reference decides a kind otherwise" % what
    dev = lref.deviation(own[unit_spec.LINK]["impulse"], exact.link_impulse)
    print("%-40s %.3g" % (what, dev))
    assert dev <= BOUND, what
    return dev


def test_spec_against_the_float64_reference(built_lib, oracle):
    worst = 0.0
    for k, (b, links) in enumerate(_scenes()):
        worst = max(worst, _compare(b, [NO_PINS, links], [0], "scene %d" % k))
    for name in link_corpus.NAMES:                         # (none left out: link_corpus.ON_A_COMPARISON)
        for tether in (False, True):
            m = link_corpus.build(name, tether)
            worst = max(worst, _compare(_pre_solve_bodies(oracle, m), [m.pins, m.links], _order(m), name + (" tethered" if tether else "")))
    print("worst %.3g" % worst)
