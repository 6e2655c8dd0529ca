"""Force fields without a GPU: phx_field_check, the single validator, rule by rule; and tests/field_spec.py, the definition the device
matches, against closed forms computed in float64."""
import ctypes as C
import itertools

import numpy as np
import pytest

import phyx_amd
from phyx_amd import uniform_field, radial_field, drag_field, field_dtype
from phyx_amd.api import rigid_body_dtype
import field_spec

F = np.float32
INVALID = -1


def _check(lib, fields, count=None):
    a = np.ascontiguousarray(fields, dtype=field_dtype).reshape(-1)
    st = lib.phx_field_check(a.ctypes.data_as(C.c_void_p), len(a) if count is None else count)
    return st, lib.phx_last_error().decode()


def _valid(kind, shape):
    region = {0: {}, 1: {"box": (-10.0, -5.0, 10.0, 5.0)}, 2: {"disc": (1.0, 2.0, 30.0)}}[shape]
    if kind == 0:
        return uniform_field(3.0, -4.0, 0.5, **region)
    if kind == 1:
        return radial_field(0.0, 50.0, -200.0, 80.0, **region)
    return drag_field(2.0, 1.0, flow=(5.0, 0.0), **region)


@pytest.mark.parametrize("kind,shape", list(itertools.product(range(3), range(3))))
def test_check_accepts_every_kind_and_shape(built_lib, kind, shape):
    st, msg = _check(built_lib, [_valid(kind, shape)])
    assert st == 0, msg
    f = _valid(kind, shape).copy()
    f["flags"] = phyx_amd.FIELD_FORCE
    f["mask"] = 4
    assert _check(built_lib, [f])[0] == 0
    phyx_amd.field_check([f])


def test_check_counts(built_lib):
    assert built_lib.phx_field_check(None, 0) == 0
    full = np.stack([_valid(k % 3, (k // 3) % 3) for k in range(phyx_amd.MAX_FIELDS)])
    assert _check(built_lib, full)[0] == 0
    over = np.concatenate([full, full[:1]])
    st, msg = _check(built_lib, over)
    assert st == INVALID and "257" in msg and "PHX_MAX_FIELDS" in msg
    st, msg = _check(built_lib, full[:1], count=-1)
    assert st == INVALID and "negative count" in msg
    assert built_lib.phx_field_check(None, 1) == INVALID
    assert "null array" in built_lib.phx_last_error().decode()


def _broken(edit):
    f = np.stack([_valid(0, 1), _valid(1, 2), _valid(2, 0)])
    edit(f)
    return f


def _set(k, name, value, index=None):
    def edit(f):
        if index is None:
            f[name][k] = value
        else:
            f[name][k][index] = value
    return edit


REJECTED = [
    ("kind 3", _set(1, "kind", 3), "field 1: unknown kind 3"),
    ("kind -1", _set(0, "kind", -1), "field 0: unknown kind -1"),
    ("shape 3", _set(2, "shape", 3), "field 2: unknown shape 3"),
    ("flag bit 2", _set(0, "flags", 2), "field 0: flags 0x2 hold an unknown bit"),
    ("flag bits 3", _set(0, "flags", 3), "unknown bit"),
    ("mask 0", _set(1, "mask", 0), "field 1: mask 0"),
    ("box min.x > max.x", _set(0, "region", 11.0, 0), "field 0: the box's min exceeds its max"),
    ("box min.y > max.y", _set(0, "region", 6.0, 1), "field 0: the box's min exceeds its max"),
    ("negative radius", _set(1, "region", -1.0, 2), "field 1: negative disc radius"),
    ("negative falloff", _set(1, "value", -0.5, 3), "field 1: negative falloff radius"),
    ("negative k_lin", _set(2, "value", -1.0, 2), "field 2: negative drag coefficient"),
    ("negative k_ang", _set(2, "value", -1.0, 3), "field 2: negative drag coefficient"),
    ("unused region word of ALL", _set(2, "region", 1.0, 0), "field 2: region[0] is unused"),
    ("unused region word of a disc", _set(1, "region", 1.0, 3), "field 1: region[3] is unused"),
    ("unused value word of UNIFORM", _set(0, "value", 1.0, 3), "field 0: value[3] is unused"),
]


@pytest.mark.parametrize("name,edit,message", REJECTED, ids=[r[0] for r in REJECTED])
def test_check_rejects(built_lib, name, edit, message):
    st, msg = _check(built_lib, _broken(edit))
    assert st == INVALID and message in msg, msg
    with pytest.raises(phyx_amd.PhxError) as e:
        phyx_amd.field_check(_broken(edit))
    assert e.value.status == INVALID


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("slot", ["region", "value"])
@pytest.mark.parametrize("index", range(4))
def test_check_rejects_a_non_finite_float_in_every_slot(built_lib, bad, slot, index):
    for k in range(3):                      # a box, a disc and ALL; a uniform, a radial and a drag: every slot, used or not
        st, msg = _check(built_lib, _broken(_set(k, slot, bad, index)))
        assert st == INVALID and "field %d: %s[%d] is not finite" % (k, slot, index) in msg, msg


def test_check_first_failure_wins(built_lib):
    f = _broken(lambda f: None)
    f["mask"][2] = 0
    f["kind"][1] = 7
    assert "field 1: unknown kind 7" in _check(built_lib, f)[1]          # list order
    f = _broken(lambda f: None)
    f["mask"][0] = 0
    f["region"][0][0] = np.nan
    assert "field 0: mask 0" in _check(built_lib, f)[1]                   # rule order within a field


# ---- the spec against closed forms in float64 -------------------------------------------------------------------------------------------
def _bodies(rows):
    """records for rows (x, y, vx, vy, w, inv_mass, inv_inertia)"""
    b = np.zeros(len(rows), dtype=rigid_body_dtype)
    for i, (x, y, vx, vy, w, m, ii) in enumerate(rows):
        b["pos"][i] = (x, y)
        b["velocity"][i] = (vx, vy)
        b["angular_velocity"][i] = w
        b["inv_mass"][i], b["inv_inertia"][i] = m, ii
    return b


def test_spec_uniform_is_what_gravity_adds():
    g, dt = F(-200.0), F(1.0 / 60.0)
    b = _bodies([(3.0, 7.0, 1.5, -2.5, 0.3, 4.0, 9.0), (0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0), (5.0, 5.0, 0.0, 0.0, 0.0, 0.0, 2.0)])
    a = field_spec.step_accelerations(np.stack([uniform_field(0.0, float(g))]), dt, b)
    # IntegrateVelocity (ref: World.cpp:44-48): ay = acceleration.y (+ gravity if invMass > 0); v.y += ay * dt
    for i in range(len(b)):
        want = F(0.0) + g if b["inv_mass"][i] > 0 else F(0.0)
        assert a[i].tobytes() == np.array([0.0, want, 0.0], dtype=np.float32).tobytes()
        assert F(b["velocity"]["y"][i]) + a[i, 1] * dt == F(b["velocity"]["y"][i]) + want * dt


def test_spec_radial_without_falloff_has_the_strength_and_points_from_the_centre():
    rng = np.random.default_rng(3)
    for strength in (250.0, -75.5):
        for _ in range(50):
            c = rng.uniform(-100, 100, 2)
            p = c + rng.uniform(-300, 300, 2)
            b = _bodies([(p[0], p[1], 0, 0, 0, 2.0, 3.0)])
            a = field_spec.step_accelerations(np.stack([radial_field(c[0], c[1], strength)]), 1.0 / 60.0, b)[0]
            mag = np.hypot(float(a[0]), float(a[1]))
            assert abs(mag - abs(strength)) <= 2 * float(np.spacing(F(abs(strength))))
            d = np.array([float(F(p[0])) - float(F(c[0])), float(F(p[1])) - float(F(c[1]))])
            d /= np.linalg.norm(d)
            got = np.array([float(a[0]), float(a[1])]) / mag
            assert np.dot(got, d) * np.sign(strength) > 1.0 - 1e-6
            assert a[2] == 0.0


def test_spec_radial_falloff_is_linear_and_ends_at_the_radius():
    f = np.stack([radial_field(0.0, 0.0, 100.0, 50.0)])
    near = field_spec.step_accelerations(f, 0.01, _bodies([(25.0, 0.0, 0, 0, 0, 1.0, 1.0)]))[0]
    assert near[0] == F(50.0) and near[1] == 0.0
    for x in (50.0, 60.0, 0.0, 2.0 ** -11):
        assert not field_spec.step_accelerations(f, 0.01, _bodies([(x, 0.0, 0, 0, 0, 1.0, 1.0)])).any()


@pytest.mark.parametrize("k,dt", [(64.0, 2.0 ** -6), (1000.0, 2.0 ** -6), (1e6, 2.0 ** -8), (7.0, 0.25)])
def test_spec_stiff_drag_brings_the_velocity_to_the_flow(k, dt):
    """k dt >= 1: after IntegrateVelocity's v += a dt the velocity is the flow, to within 1 ulp of the flow.  The cases are those in
    which float32 can say so: dt a power of two (c = 1 / dt, a = (flow - v) c and a dt are then exact scalings) and v between flow / 2
    and 2 flow (flow - v is then exact, Sterbenz) — v + (flow - v) has nothing left to round.  The angular flow is 0 and 0 - w is always
    exact, so w ends at exactly 0 for any w."""
    assert k * dt >= 1.0
    rng = np.random.default_rng(11)
    dt = F(dt)
    for _ in range(50):
        flow = rng.uniform(1.0, 50.0, 2) * rng.choice([-1.0, 1.0], 2)
        v = np.array([float(F(flow[0])), float(F(flow[1]))]) * rng.uniform(0.5, 2.0, 2)
        w = rng.uniform(-500, 500)
        b = _bodies([(1.0, 2.0, v[0], v[1], w, 5.0, 6.0)])
        a = field_spec.step_accelerations(np.stack([drag_field(k, k, flow=flow)]), dt, b)[0]
        got = (F(v[0]) + a[0] * dt, F(v[1]) + a[1] * dt, F(w) + a[2] * dt)          # IntegrateVelocity's v += a * dt
        for g, want in zip(got, (flow[0], flow[1], 0.0)):
            assert abs(float(g) - float(F(want))) <= float(np.spacing(F(abs(want)))), (g, want)


@pytest.mark.parametrize("k,dt", [(60.0, 1.0 / 60.0), (100.0, 1.0 / 60.0), (1e6, 1.0 / 240.0)])
def test_spec_stiff_drag_in_general_lands_within_the_roundings_of_its_four_operations(k, dt):
    """Any dt, any v.  One ulp of the flow itself is not reachable where v dwarfs it: the cancellation v + (flow - v) is rounded at
    v's magnitude.  The bound that holds, with M = max(|v|, |flow|) and u = 2^-24: flow - v, c = 1 / dt, * c and * dt round once each,
    4 u relative on a dt, whose size is at most |flow - v| <= 2 M: 8 u M < 8 ulp(M); the final v + rounds at the result's magnitude,
    half an ulp(M) more.  So the velocity ends within 8.5 ulp(M) of the flow."""
    assert k * dt >= 1.0
    rng = np.random.default_rng(12)
    dt = F(dt)
    for _ in range(50):
        flow = rng.uniform(-50, 50, 2)
        v = rng.uniform(-500, 500, 3)
        b = _bodies([(1.0, 2.0, v[0], v[1], v[2], 5.0, 6.0)])
        a = field_spec.step_accelerations(np.stack([drag_field(k, k, flow=flow)]), dt, b)[0]
        got = (F(v[0]) + a[0] * dt, F(v[1]) + a[1] * dt, F(v[2]) + a[2] * dt)
        for g, want, start in zip(got, (flow[0], flow[1], 0.0), v):
            assert abs(float(g) - float(F(want))) <= 8.5 * float(np.spacing(F(max(abs(start), abs(want)))))


def test_spec_half_drag_halves_the_speed():
    dt = F(1.0 / 64.0)
    b = _bodies([(0.0, 0.0, 48.0, -16.0, 4.0, 1.0, 1.0)])
    a = field_spec.step_accelerations(np.stack([drag_field(32.0, 32.0)]), dt, b)[0]          # k dt = 0.5, all powers of two: exact
    assert (F(48.0) + a[0] * dt, F(-16.0) + a[1] * dt, F(4.0) + a[2] * dt) == (24.0, -8.0, 2.0)


def test_spec_force_scales_by_the_inverse_masses():
    b = _bodies([(10.0, 0.0, 3.0, 4.0, 5.0, 0.25, 0.125)])
    for mk in (lambda **kw: uniform_field(8.0, -16.0, 32.0, **kw), lambda **kw: radial_field(0.0, 0.0, 64.0, **kw), lambda **kw: drag_field(2.0, 4.0, **kw)):
        plain = field_spec.step_accelerations(np.stack([mk()]), 0.125, b)[0]
        force = field_spec.step_accelerations(np.stack([mk(force=True)]), 0.125, b)[0]
        assert force.tobytes() == (plain * np.array([0.25, 0.25, 0.125], dtype=np.float32)).tobytes()
        assert plain.any()


def test_spec_who_is_affected():
    f = np.stack([uniform_field(1.0, 2.0, 3.0, mask=6)])
    b = _bodies([(0, 0, 0, 0, 0, 1.0, 1.0)] * 4 + [(0, 0, 0, 0, 0, 0.0, 1.0)])
    assert not field_spec.step_accelerations(f, 0.1, b).any()                                 # no column: category 1 misses mask 6
    a = field_spec.step_accelerations(f, 0.1, b, categories=[1, 2, 4, 8, 2])
    assert a[:, 0].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]                                      # ... and inv_mass 0 is never written
    nan = _bodies([(np.nan, 0.0, 0, 0, 0, 1.0, 1.0)])
    assert field_spec.step_accelerations(np.stack([uniform_field(1.0, 0.0)]), 0.1, nan)[0, 0] == 1.0
    for region in ({"box": (-1.0, -1.0, 1.0, 1.0)}, {"disc": (0.0, 0.0, 5.0)}):
        assert not field_spec.step_accelerations(np.stack([uniform_field(1.0, 0.0, **region)]), 0.1, nan).any()


def test_spec_honours_list_order():
    """float32 addition does not associate: the same two fields in the other order give other bytes, and pending comes first."""
    big, small = uniform_field(2.0 ** 25, 0.0), uniform_field(1.0, 0.0)
    b = _bodies([(0, 0, 0, 0, 0, 1.0, 1.0)])
    b["acceleration"]["x"][0] = -(2.0 ** 25)
    ab = field_spec.step_accelerations(np.stack([big, small]), 0.1, b)[0]
    ba = field_spec.step_accelerations(np.stack([small, big]), 0.1, b)[0]
    assert ab[0] == 1.0 and ba[0] == 0.0                       # (-2^25 + 2^25) + 1  against  (-2^25 + 1) + 2^25, whose first sum rounds to -2^25
    assert ab.tobytes() != ba.tobytes()


def test_spec_impulse_through_the_centre_turns_nothing():
    b = _bodies([(10.0, 20.0, 1.0, 2.0, 0.5, 0.5, 0.25), (0.0, 0.0, 1.0, 2.0, 0.5, 0.0, 0.25)])
    assert field_spec.impulse(b[0], 4.0, -6.0, 10.0, 20.0) == (3.0, -1.0, 0.5)
    vx, vy, w = field_spec.impulse(b[0], 0.0, 8.0, 12.0, 20.0)             # r = (2, 0), J = (0, 8): r x J = 16, counter-clockwise
    assert (vx, vy, w) == (1.0, 6.0, 0.5 - 0.25 * 16.0)                    # ... so the clockwise-positive w drops
    assert field_spec.impulse(b[1], 4.0, -6.0, 3.0, 3.0) == (1.0, 2.0, 0.5)            # inv_mass 0: skipped


def test_helpers_build_the_records_the_header_describes():
    f = radial_field(1.0, 2.0, -3.0, 4.0, disc=(5.0, 6.0, 7.0), mask=12, force=True)
    assert f.dtype == field_dtype and f.tobytes() == np.array([1, 2, 12, 1], dtype="<i4").tobytes() + np.array([5, 6, 7, 0, 1, 2, -3, 4], dtype="<f4").tobytes()
    f = drag_field(0.5, 0.25, flow=(9.0, 8.0), box=(1.0, 2.0, 3.0, 4.0))
    assert f.tobytes() == np.array([2, 1, 0xFFFFFFFF, 0], dtype="<u4").tobytes() + np.array([1, 2, 3, 4, 9, 8, 0.5, 0.25], dtype="<f4").tobytes()
    with pytest.raises(ValueError):
        uniform_field(1.0, 0.0, box=(0, 0, 1, 1), disc=(0, 0, 1))
    with pytest.raises(TypeError):
        phyx_amd.field_check([np.zeros(3)])
