"""The pin corpus without a GPU (tests/pin_corpus.py): every motif's claims proved with the host-only schedule builder and
pin_spec.prestep; the spec (tests/pin_spec.py) held to the independent float64 reference (tests/pin_reference.py) on every motif and on
200 random chains; the reference's one sign convention pinned to the integrators; three checks that need no reference at all; and the
singular pin (pin_spec.py DET_FLOOR).

The bound of a comparison with the reference is never a number written here: it is 8 x the deviation of the reference's own float32 run
from its float64 run on the same input, floored at one float32 ulp (the spec's Cramer form and the reference's LU round differently, by a
few ulps per sweep), in the metric of pin_reference.deviation."""
import numpy as np
import pytest

from phyx_amd import api
import pin_corpus
from pin_corpus import CONSERVING, INACTIVE, MARGIN, ONE_PIN, U, ULP, check_momentum, check_residual, check_the_anchor_is_followed
import pin_reference as ref
import pin_spec
import unit_reference
import unit_spec

DT = pin_corpus.DT


def _pre_solve_bodies(oracle, m, gravity=None):
    """the motif's bodies as the pin pass finds them: after the oracle's IntegrateVelocity (pre_solve; no contact forms)"""
    ow = m.oracle_world(oracle, gravity)
    ow.pre_solve(DT)
    assert len(ow.manifolds()) == 0, "%s: bodies touch" % m.name
    return ow.bodies().copy()


def _initial_bodies(oracle, m, gravity=None):
    ow = m.oracle_world(oracle, gravity)                 # (kept alive until its bodies are copied)
    return ow.bodies().copy()


def _order(m, cap=None):
    b1, b2, st = m.graph()
    return api.pin_schedule(b1, b2, st, group_pins=cap or m.cap or 256)


def noise_and_deviation(bodies, pins, order, iterations, q):
    """-> (the float64 result, the float32 result, the reference's own float32-vs-float64 deviation floored at an ulp, the deviation
    of q from float64)"""
    exact = unit_reference.solve(bodies, [pins], order, DT, iterations, np.float64)
    single = unit_reference.solve(bodies, [pins], order, DT, iterations, np.float32)
    return exact, single, max(ref.deviation(single.q, exact.q), ULP), ref.deviation(q, exact.q)


# ---- the claims ----
@pytest.mark.parametrize("name", pin_corpus.NAMES)
def test_motif_reaches_what_it_claims(built_lib, oracle, name):
    m = pin_corpus.build(name)
    b1, b2, st = m.graph()
    cap = m.cap or 256
    s = api.pin_schedule(b1, b2, st, group_pins=cap)
    pin_corpus.check_schedule(b1, b2, st, s, cap, name)
    assert pin_corpus.shape_of(s) == m.shape, "(classes, group sizes, LDS groups)"
    if name in pin_corpus.MULTI:
        one = api.pin_schedule(b1, b2, st, group_pins=1)
        pin_corpus.check_schedule(b1, b2, st, one, 1, name)
        if name in pin_corpus.CONNECTED:
            assert one["lds_groups"] == 0 and len(one["group_offsets"]) == 2, "a cap of 1 sends a connected motif whole to the trailing group"
    assert all(r[2] != 0.0 for r in m.rows), "a motif's bodies start turned"
    bodies = _initial_bodies(oracle, m)
    pins = m.pins
    beta = pin_spec.BETA / pin_spec.F(DT)
    for k in range(len(pins)):
        p = pin_spec.prestep(bodies, pins[k], beta)
        assert (p.active, p.write_a, p.write_b) == m.flags[k], "pin %d of %s: (active, write_a, write_b)" % (k, name)
        assert k not in m.k12_zero or (p.active and p.k12 == 0), "pin %d of %s: k12" % (k, name)
        k11, k12, k22 = np.float32(p.k11), np.float32(p.k12), np.float32(p.k22)
        assert p.active == bool(k11 * k22 - k12 * k12 > 0) or name in pin_corpus.SINGULAR, "only a singular pin changes under the floor"
        assert not m.noise_det or k11 * k22 - k12 * k12 > 0, "%s: the det expression is not positive, the motif does not reach the floor" % name


def test_the_lists_cover_the_corpus():
    assert set(pin_corpus.CONNECTED) >= {"triangle", "ring5", "double_pin", "grid8x8", "hub5", "hub64", "hub65", "hub130", "chain256", "chain257", "warm"}
    assert set(pin_corpus.MULTI) - set(pin_corpus.CONNECTED) >= {"static_hub300", "own_statics256", "inactive_beside_active", "kinematic_anchor"}
    assert max(len(pin_corpus.build(n).rows) for n in pin_corpus.NAMES) <= 520


def free_steps(oracle, m, steps):
    """`steps` steps of the oracle World with the spec's pin pass between pre_solve and IntegratePosition (no contact may form: there
    is nothing else to solve) -> (the world, the pins with their impulses)"""
    ow, pins = m.oracle_world(oracle), m.pins
    order = _order(m)["order"]
    for s in range(steps):
        ow.pre_solve(DT)
        assert len(ow.manifolds()) == 0, "%s: bodies touch at step %d" % (m.name, s)
        unit_spec.solve_units(ow.bodies(), [pins], order, DT, 8)
        ow.integrate_position(DT)
    return ow, pins


@pytest.mark.parametrize("name", pin_corpus.NAMES)
def test_no_contact_forms_in_the_steps_a_motif_runs(built_lib, oracle, name):
    m = pin_corpus.build(name)
    ow, pins = free_steps(oracle, m, m.steps + 1)
    b = ow.bodies()
    assert np.isfinite(b["pos"]["x"]).all() and np.isfinite(b["velocity"]["x"]).all() and np.isfinite(pins["impulse"]).all()


def test_the_pinned_bodies_follow_a_kinematic_anchor(built_lib, oracle):
    m = pin_corpus.build("kinematic_anchor")
    start = _initial_bodies(oracle, m)
    ow, _ = free_steps(oracle, m, m.steps)
    check_the_anchor_is_followed(m, start, ow.bodies().copy(), m.steps)


# ---- the spec against the float64 reference ----
@pytest.mark.parametrize("iterations", [1, 8])
@pytest.mark.parametrize("name", pin_corpus.NAMES)
def test_spec_against_the_float64_reference(built_lib, oracle, name, iterations):
    m = pin_corpus.build(name)
    before = _pre_solve_bodies(oracle, m)
    order = _order(m)["order"]
    bodies, pins = before.copy(), m.pins
    unit_spec.solve_units(bodies, [pins], order, DT, iterations)
    exact, single, noise, dev = noise_and_deviation(before, m.pins, order, iterations, ref.velocities(bodies))
    impulse_noise = max(ref.deviation(single.pin_impulse, exact.pin_impulse), ULP)
    print("%-24s n=%d noise %.3g spec %.3g ratio %.2f%s" % (name, iterations, noise, dev, dev / noise, " x" if noise > pin_corpus.EXCLUDE_ABOVE else ""))
    assert exact.pin_active.tolist() == [f[0] for f in m.flags], "the reference finds the same pins well posed"
    if noise > pin_corpus.EXCLUDE_ABOVE:
        assert name in pin_corpus.MAY_BE_EXCLUDED, "%s is too ill-conditioned for the comparison (%.3g): only %s may be" % (name, noise, pin_corpus.MAY_BE_EXCLUDED)
        return
    assert dev <= MARGIN * noise
    assert ref.deviation(pins["impulse"], exact.pin_impulse) <= MARGIN * impulse_noise, "the accumulated impulses"


def test_spec_against_the_float64_reference_on_random_chains(built_lib, oracle):
    for iterations in (1, 8):
        worst_noise = worst_dev = worst_ratio = 0.0
        for seed in range(200):
            m = pin_corpus.random_chain(seed)
            before = _initial_bodies(oracle, m, 0.0)
            order = _order(m)["order"]
            bodies, pins = before.copy(), m.pins
            unit_spec.solve_units(bodies, [pins], order, DT, iterations)
            _, _, noise, dev = noise_and_deviation(before, m.pins, order, iterations, ref.velocities(bodies))
            assert noise <= pin_corpus.EXCLUDE_ABOVE, "chain %d is ill-conditioned" % seed
            assert dev <= MARGIN * noise, "chain %d" % seed
            worst_noise, worst_dev, worst_ratio = max(worst_noise, noise), max(worst_dev, dev), max(worst_ratio, dev / noise)
        print("200 random chains, n=%d: spec %.3g, the reference's own float32 %.3g (%.2fx); worst single chain %.2fx"
              % (iterations, worst_dev, worst_noise, worst_dev / worst_noise, worst_ratio))
        assert worst_dev <= MARGIN * worst_noise


# ---- the sign convention ----
def _carried_point(pos, xv, yv, a):
    return np.array([pos[0] + xv[0] * a[0] + yv[0] * a[1], pos[1] + xv[1] * a[0] + yv[1] * a[1]], dtype=np.float64)


def _frame(b, i=0):
    return ((float(b["pos"]["x"][i]), float(b["pos"]["y"][i])), (float(b["xv"]["x"][i]), float(b["xv"]["y"][i])),
            (float(b["yv"]["x"][i]), float(b["yv"]["y"][i])))


@pytest.mark.parametrize("integrator", ["oracle", "spec"])
@pytest.mark.parametrize("v,w", [((2.0, -1.0), 1.5), ((0.0, 0.0), -2.0), ((-1.0, 3.0), 0.0)])
def test_point_jacobian_is_what_the_integrators_do(oracle, integrator, v, w):
    """A body-frame point carried through IntegratePosition moves by J q dt to first order in dt: that fixes the sign of the
    reference's one convention row from the engine's own integrator (and from the spec's stepper)."""
    dt, a = 1.0 / 1024.0, (1.5, -0.75)
    ow = oracle.OracleWorld(0.0)
    ow.add_body(3.0, 4.0, 0.6, 3.0, 1.0)
    b = ow.bodies()
    b["velocity"]["x"][0], b["velocity"]["y"][0], b["angular_velocity"][0] = v[0], v[1], w
    start = _frame(b)
    p0 = _carried_point(*start, a)
    if integrator == "oracle":
        ow.integrate_position(dt)
        end = _frame(ow.bodies())
    else:
        copy = b.copy()
        unit_spec.step_free(copy, [], [], dt, 0.0)
        end = _frame(copy)
    got = (_carried_point(*end, a) - p0) / dt
    r = p0 - np.array(start[0])
    want = ref.point_jacobian(r) @ np.array([v[0], v[1], w])
    # second order in dt: the centripetal term w^2 |r| dt / 2; float32 poses: a few roundings of |pos| + |r|, divided by dt
    tol = w * w * np.hypot(*r) * dt + 8 * U * (np.hypot(*start[0]) + np.hypot(*r)) / dt
    print("carried %s, J q %s, tolerance %.3g" % (got, want, tol))
    assert np.abs(got - want).max() <= tol
    assert w == 0.0 or np.abs(2.0 * w * r).min() > 10 * tol, "the test could not tell a wrong sign"


# ---- the pendulum's release height ----
def test_the_spec_pendulum_never_rises_above_its_release():
    """A wrong angular sign pumps energy in: the pendulum climbs.  The float64 stepper of the reference bounds how far the discrete
    scheme itself lets it rise above the height it was released at; the spec may exceed that by float32's rounding of the
    position over the run, 300 steps of half an ulp of 300 (2^-16) each."""
    steps, top = 300, 300.0
    rows, pins = pin_spec.chain(1, spacing=10.0)
    bodies = pin_spec.make_bodies(rows)
    state, pins64 = ref.free_state(bodies, pins)
    release = float(bodies["pos"]["y"][0])
    rise = rise64 = -np.inf
    lowest = np.inf
    for _ in range(steps):
        unit_spec.step_free(bodies, [pins], [0], DT, -200.0, iterations=8)
        ref.step_free(state, pins64, [0], DT, -200.0, iterations=8)
        rise, rise64 = max(rise, float(bodies["pos"]["y"][0]) - release), max(rise64, float(state["pos"][0, 1]) - release)
        lowest = min(lowest, float(bodies["pos"]["y"][0]))
    margin = steps * 2.0 ** -16
    print("rise above the release height: spec %.6g, float64 %.6g, margin %.3g" % (rise, rise64, margin))
    assert lowest < top - 4.0, "the pendulum never swung"
    assert rise <= max(rise64, 0.0) + margin


# ---- checks without a reference ----
@pytest.mark.parametrize("name", ONE_PIN + tuple("random%d" % s for s in range(20)))
def test_one_sweep_of_one_pin_leaves_no_residual(built_lib, oracle, name):
    m = pin_corpus.random_chain(int(name[6:]), links=1) if name.startswith("random") else pin_corpus.build(name)
    before = _pre_solve_bodies(oracle, m)
    after, pins = before.copy(), m.pins
    assert len(pins) == 1 and not pins["impulse"].any()
    unit_spec.solve_units(after, [pins], [0], DT, 1)
    check_residual(before, after, m.pins[0])


def test_the_conserving_motifs():
    assert set(CONSERVING) >= {"pair", "triangle", "ring5", "double_pin", "double_pin_swapped", "grid8x8", "hub5", "hub63", "hub64", "hub65", "hub130"}


@pytest.mark.parametrize("name", CONSERVING)
def test_the_pass_conserves_momentum(built_lib, oracle, name):
    m = pin_corpus.build(name)
    before = _pre_solve_bodies(oracle, m, gravity=0.0)
    after, pins = before.copy(), m.pins
    unit_spec.solve_units(after, [pins], _order(m)["order"], DT, 8)
    assert after["velocity"].tobytes() != before["velocity"].tobytes()
    check_momentum(m, before, after, pins["impulse"], 8)


@pytest.mark.parametrize("name", INACTIVE)
def test_an_inactive_pin_changes_nothing(built_lib, oracle, name):
    m = pin_corpus.build(name)
    before = _pre_solve_bodies(oracle, m)
    after, pins = before.copy(), m.pins
    assert pins["impulse"].any()
    unit_spec.solve_units(after, [pins], [0], DT, 8)
    assert after.tobytes() == before.tobytes()
    assert not pins["impulse"].any(), "an inactive pin reads impulse 0"


# ---- the singular pin ----
@pytest.mark.parametrize("make", [pin_corpus.random_axle, pin_corpus.random_axle_pair])
def test_a_singular_pin_is_inactive(built_lib, oracle, make):
    """200 wheels on fixed axles pinned off-centre to the world, 200 pairs of wheels pinned on the line through their axles: det is 0 in
    real arithmetic and rounding noise in float32.  `det > 0` took the noise for a determinant in a third of them."""
    beta = pin_spec.BETA / pin_spec.F(DT)
    noisy = 0
    for seed in range(200):
        m = make(seed)
        before = _initial_bodies(oracle, m, 0.0)
        p = pin_spec.prestep(before, m.pins[0], beta)
        noisy += bool(np.float32(p.k11) * np.float32(p.k22) - np.float32(p.k12) * np.float32(p.k12) > 0)
        after, pins = before.copy(), m.pins
        unit_spec.solve_units(after, [pins], [0], DT, 8)
        assert not p.active, "case %d is active" % seed
        assert after.tobytes() == before.tobytes(), "case %d: the bodies changed" % seed
        assert not pins["impulse"].any(), "case %d: the impulse reads %s" % (seed, pins["impulse"])
        assert not unit_reference.solve(before, [m.pins], [0], DT, 8).pin_active[0], "the reference finds case %d well posed" % seed
    print("%s: det > 0 in %d of 200" % (make.__name__, noisy))
    assert noisy > 0, "the cases never produce a positive det: they do not test the floor"


def test_a_wheel_pinned_to_a_dynamic_body_is_active(built_lib, oracle):
    m = pin_corpus.build("axle_dynamic")
    before = _pre_solve_bodies(oracle, m)
    after, pins = before.copy(), m.pins
    unit_spec.solve_units(after, [pins], _order(m)["order"], DT, 8)
    assert pins["impulse"].all() and after["angular_velocity"][0] != before["angular_velocity"][0]
    assert (after["velocity"][0], after["pos"][0]) == (before["velocity"][0], before["pos"][0]), "the axle itself does not move"
