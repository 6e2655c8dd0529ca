"""Materials without a GPU: tests/material_spec.py against the oracle where the two overlap (every material the default), the exact
fmaf emulation, hand-checked RefreshJoints cases where a restitution changes dstVelocity, the pair rule and material_dtype."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import material_spec as spec
import path_edges as pe
import phyx_amd
from phyx_amd.api import material_dtype
from test_solver_gpu import _random_state

F32 = np.float32


def _static(bodies):
    return ((bodies["inv_mass"] == 0) & (bodies["inv_inertia"] == 0)).astype(np.uint8)


def _colours(bodies, joints):
    order, offs = phyx_amd.schedule_colours(joints["body1"], joints["body2"], _static(bodies), joints["contact_point_index"])
    return order, offs, np.array([0, len(joints)], dtype=np.int32)


def _groups(bodies, joints):
    g = phyx_amd.schedule_groups(joints["body1"], joints["body2"], _static(bodies), joints["contact_point_index"])
    return g["order"], g["colour_offsets"], g["group_offsets"]


def _random(seed, nb=300, nj=700, static_frac=0.05):
    rng = np.random.default_rng(seed)
    b, c, j = _random_state(rng, nb, nj, static_frac)
    j["friction_acc"] = rng.uniform(-0.02, 0.02, nj)
    b["angular_velocity"] = np.where(_static(b) != 0, 0.0, rng.uniform(-0.5, 0.5, nb))
    b["displacing_velocity"]["x"] = np.where(_static(b) != 0, 0.0, rng.uniform(-0.1, 0.1, nb))
    return b, c, j


STATES = {
    "random_a": lambda: _random(11),
    "random_b": lambda: _random(12, 500, 1500, 0.1),
    "tail_of_2": lambda: pe.tail_state("tail_of_2"),
    "lds_units_256": lambda: pe.lds_state("units_256"),
}


@pytest.fixture(params=[0, 1], ids=["source", "fused"])
def arith(request, oracle):
    prev = oracle.set_arith(request.param)
    yield request.param
    oracle.set_arith(prev)


@pytest.mark.parametrize("builder", ["colours", "groups"])
@pytest.mark.parametrize("name", sorted(STATES))
def test_spec_is_the_oracle_at_default_materials(oracle, arith, name, builder):
    """Every material the default (mu = 0.3, e = 0): material_spec.solve_grouped and the oracle's grouped solve leave the same bytes in
    bodies and joints, on the host builders' schedules, in both arithmetic forms."""
    bodies, cps, joints = STATES[name]()
    order, offs, groups = (_colours if builder == "colours" else _groups)(bodies, joints)
    mu, e = spec.joint_values(spec.defaults(len(bodies)), joints)
    assert (mu == F32(0.3)).all() and (e == 0).all()
    ob, oj = bodies.copy(), joints.copy()
    oracle.solver_solve_grouped(ob, cps, oj, order, offs, groups, 12, 6, oracle.STAG_COLOUR_SYNC)
    sb, sj = bodies.copy(), joints.copy()
    spec.solve_grouped(sb, cps, sj, order, offs, groups, 12, 6, mu, e, fused=arith)
    assert sj.tobytes() == oj.tobytes()
    assert sb.tobytes() == ob.tobytes()
    assert sb.tobytes() != bodies.tobytes()                       # (the solve did something)


def test_mixed_materials_change_the_solve():
    """Ice, rubber and defaults mixed: the spec's solve differs from the default one, and it stays finite."""
    bodies, cps, joints = _random(13)
    order, offs, groups = _colours(bodies, joints)
    rng = np.random.default_rng(3)
    mat = spec.materials(len(bodies), rng.choice([0.0, 0.3, 1.0], len(bodies)), rng.choice([0.0, 0.8], len(bodies)))
    mu, e = spec.joint_values(mat, joints)
    a, aj = bodies.copy(), joints.copy()
    spec.solve_grouped(a, cps, aj, order, offs, groups, 12, 6, mu, e)
    d, dj = bodies.copy(), joints.copy()
    spec.solve_grouped(d, cps, dj, order, offs, groups, 12, 6, *spec.joint_values(spec.defaults(len(bodies)), joints))
    assert a.tobytes() != d.tobytes()
    assert np.isfinite(a["velocity"]["x"]).all() and np.isfinite(aj["friction_acc"]).all()
    # friction 0 on both bodies: no friction impulse at all
    free = mu == 0
    assert free.any() and (aj["friction_acc"][free] == 0).all()


def _libm_fmaf():
    path = ctypes.util.find_library("m")
    if not path:
        return None
    f = ctypes.CDLL(path).fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return f


def test_fmaf_emulation_is_exact():
    """spec.fmaf against libm's fmaf on random, cancelling and tie-prone float32 triples."""
    f = _libm_fmaf()
    if f is None:
        pytest.skip("no libm on this host")
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(F32) * F32(3)
    b = rng.standard_normal(4000).astype(F32)
    c = rng.standard_normal(4000).astype(F32)
    c[:1000] = -(a[:1000] * b[:1000]).astype(F32)                  # cancellation: the rounding of the product decides
    a[1000:2000] = F32(1) + F32(2.0 ** -23) * rng.integers(0, 8, 1000).astype(F32)
    b[1000:2000] = F32(1) + F32(2.0 ** -23) * rng.integers(0, 8, 1000).astype(F32)
    got = spec.fmaf(a, b, c)
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)
    assert got.tobytes() == want.tobytes()
    assert (got != ((a * b).astype(F32) + c).astype(F32)).any()    # (the unfused form differs somewhere: the test has teeth)


def test_refresh_restitution_hand_cases(oracle):
    """dstVelocity = depth < 1 ? max(dv - 1, 0) - 0.1 : max(dv - 1, 0), dv = -e (relV . n), checked by hand."""
    q = (1.0, 0.1, 0.0, 0.0)           # im, ii, pos
    d0 = (0.0, 0.0)
    n = (0.0, 1.0)
    # body 1 falls onto body 2 at 10 units/s along -n: relV . n = -10
    v1, v2 = (0.0, -10.0, 0.0), (0.0, 0.0, 0.0)
    assert spec.dst_velocity(v1, v2, q, q, d0, (0.0, 0.5), n, 0.5)[0] == F32(4.0) - F32(0.1)       # dv = 5: 4, depth 0.5 < 1
    assert spec.dst_velocity(v1, v2, q, q, d0, (0.0, 1.5), n, 0.5)[0] == F32(4.0)                  # depth 1.5: no -0.1
    assert spec.dst_velocity(v1, v2, q, q, d0, (0.0, 0.5), n, 0.0)[0] == F32(-0.1)                 # e = 0: the reference
    assert spec.dst_velocity(v1, v2, q, q, d0, (0.0, 0.5), n, 0.05)[0] == F32(-0.1)                # dv = 0.5 < 1: nothing
    assert spec.dst_velocity(v1, v2, q, q, d0, (0.0, 0.5), n, 1.0)[0] == F32(9.0) - F32(0.1)
    # separating: relV . n = +10 -> dv < 0 -> 0
    assert spec.dst_velocity((0.0, 10.0, 0.0), v2, q, q, d0, (0.0, 0.5), n, 1.0)[0] == F32(-0.1)
    # spin: pv1.x = (pos1.y - p1.y) * w1 + v1.x; contact point 2 above body 1's centre, normal along x
    v1 = (0.0, 0.0, -4.0)            # p1 = (0, 2): pv1.x = (0 - 2) * -4 = 8, relV . n = 8 along n = (-1, 0): -8
    got = spec.dst_velocity(v1, v2, q, (1.0, 0.1, 0.0, 3.0), (0.0, 2.0), (0.0, -1.0), (-1.0, 0.0), 0.5)[0]
    assert got == F32(3.0) - F32(0.1)
    # e == 0 gives the oracle's RefreshJoints whatever the velocities, NaN included
    bodies = np.zeros(2, dtype=phyx_amd.rigid_body_dtype)
    bodies["inv_mass"], bodies["inv_inertia"] = 1.0, 0.1
    bodies["pos"]["y"] = [0.0, 0.5]
    bodies["velocity"]["y"] = [np.nan, 3.0]
    cps = np.zeros(1, dtype=phyx_amd.contact_point_dtype)
    cps["normal"]["y"] = 1.0
    j = np.zeros(1, dtype=phyx_amd.contact_joint_dtype)
    j["body2"] = 1
    ref = oracle.refresh_joint(bodies, cps, j[0])
    got = spec.dst_velocity((0.0, np.nan, 0.0), (0.0, 3.0, 0.0), (1.0, 0.1, 0.0, 0.0), (1.0, 0.1, 0.0, 0.5), (0.0, 0.0), (0.0, 0.0), (0.0, 1.0), 0.0)
    assert got.tobytes() == ref[14:15].tobytes()


def test_pair_rule():
    """mu = (fa + fb) * 0.5, e = max: exact on equal values (default bodies: exactly 0.3 and 0), symmetric, one rounding."""
    vals = np.array([0.0, 0.05, 0.3, 0.7, 1.0, 3.3, 1e6], dtype=F32)
    m = spec.materials(len(vals), vals, np.clip(vals, 0, 1))
    mu, e = spec.pair_values(m, m)
    assert mu.tobytes() == vals.tobytes() and e.tobytes() == np.clip(vals, 0, 1).astype(F32).tobytes()
    d = spec.defaults(1)
    mu, e = spec.pair_values(d[0], d[0])
    assert mu == F32(0.3) and e == 0 and not np.signbit(e)
    a, b = spec.materials(1, 0.1, 0.2)[0], spec.materials(1, 0.2, 0.8)[0]
    assert spec.pair_values(a, b) == spec.pair_values(b, a)
    assert spec.pair_values(a, b)[0] == (F32(0.1) + F32(0.2)) * F32(0.5) and spec.pair_values(a, b)[1] == F32(0.8)


def test_state_transforms():
    m = spec.materials(4, [0.0, 0.1, 0.2, 0.3], [0.0, 0.5, 1.0, 0.0])
    assert spec.spawn(m, 2)[4:].tobytes() == spec.defaults(2).tobytes()
    assert spec.remove(m, [1, 0, 1, 0]).tobytes() == m[[0, 2]].tobytes()
    assert spec.set_state(3).tobytes() == spec.defaults(3).tobytes()
    assert spec.valid([0, 1e6, -1e-9, np.nan, np.inf], [0, 1, 0, 0, 0]).tolist() == [True, True, False, False, False]
    assert spec.valid([0, 0, 0], [1.0001, -0.0, np.nan]).tolist() == [False, True, False]


def test_material_dtype():
    assert material_dtype.itemsize == 8
    assert material_dtype.names == ("friction", "restitution")
    assert material_dtype.fields["restitution"][1] == 4
    assert phyx_amd.material_dtype is material_dtype
