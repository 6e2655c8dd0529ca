"""tests/sensor_spec.py against the oracle World, on the CPU: with every flag 0, sensor_spec.refresh is the oracle's RefreshContactJoints byte
for byte on the state a tag twin reconstructs, every step; with random flags it keeps the invariants the header states."""
import numpy as np
import pytest

import sensor_spec as spec
from helpers import oracle_world
from phyx_amd import scenes

STEPS = 40
N_BODIES = 1 + 3 * 60


def _piles():
    return scenes.piles(3, 60, ymax=260.0)


def _twin_steps(scene, steps):
    """Step two identical oracle worlds A and T in lockstep; T's joints carry tags through every pre_solve.  Yields, per step,
    (manifolds, reconstructed cps, A's joints of the step before, A's cps, A's joints) — copies."""
    A, T = oracle_world(scene), oracle_world(scene)
    for s in range(steps):
        prev = A.joints().copy()
        tj = T.joints()
        assert tj.tobytes() == prev.tobytes(), "the twin left its lockstep before step %d" % s
        saved_n, saved_f = tj["normal_acc"].copy(), tj["friction_acc"].copy()
        tj["friction_acc"][:] = spec.tags(len(tj))
        A.pre_solve()
        T.pre_solve()
        m, tj = A.manifolds().copy(), T.joints()
        assert T.manifolds().tobytes() == m.tobytes()
        recon, old = spec.tag_twin_reconstruct(m, T.contact_points(), tj, A.contact_points())
        tj["friction_acc"][:] = np.where(old >= 0, saved_f[np.maximum(old, 0)], np.float32(0)) if len(saved_f) else np.float32(0)
        assert (tj["normal_acc"] == (np.where(old >= 0, saved_n[np.maximum(old, 0)], np.float32(0)) if len(saved_n) else 0)).all()
        yield m, recon, prev, A.contact_points().copy(), A.joints().copy()
        A.solve_and_integrate()
        T.solve_and_integrate()


@pytest.fixture(scope="module")
def states():
    return list(_twin_steps(_piles(), STEPS))


def test_refresh_is_the_oracles(states):
    """scenes.piles(3, 60, ymax=260.0), 40 steps: refresh(manifolds, reconstructed cps, the joints of the step before, flags = 0) equals the
    oracle World's joints and contact points byte for byte in every step, and some step deletes and creates joints in one refresh (the
    swap-remove order is exercised with the new joints behind the old ones)."""
    both = 0
    for s, (m, recon, prev, cps, joints) in enumerate(states):
        st = {}
        got_cps, got_joints = spec.refresh(m, recon, prev, spec.defaults(N_BODIES), st)
        assert got_joints.tobytes() == joints.tobytes(), "joints differ at step %d" % s
        assert got_cps.tobytes() == cps.tobytes(), "contact points differ at step %d" % s
        both += st["created"] > 0 and st["deleted"] > 0
    assert both > 0, "no step had dead and new joints in the same refresh"
    assert len(states[-1][4]) > 0


def test_refresh_properties_with_random_flags(states):
    """Random flags on those states: every live slot of a sensor manifold is -1; the other live slots and the joints are a bijection with
    matching bodies; the joint count is the number of non-sensor live slots."""
    rng = np.random.default_rng(5)
    n = N_BODIES
    sensors_seen = 0
    for s, (m, recon, prev, _, _) in enumerate(states):
        flags = (rng.random(n) < 0.2).astype(np.uint32)
        cps, joints = spec.refresh(m, recon, prev, flags)
        sens = spec.sensor_manifolds(flags, m)
        sslots = spec.sensor_slots(flags, m)
        assert (cps["solver_index"][sslots] == -1).all(), "step %d" % s
        sensors_seen += len(sslots)
        free = spec.live_slots(m[~sens]) if len(m) else np.zeros(0, dtype=np.int64)
        assert len(joints) == len(free), "step %d" % s
        si = cps["solver_index"][free].astype(np.int64)
        assert sorted(si.tolist()) == list(range(len(joints))), "step %d: slots and joints are no bijection" % s
        assert (joints["contact_point_index"][si] == free).all(), "step %d" % s
        man = m[free // 2]
        assert (joints["body1"][si] == man["body1"]).all() and (joints["body2"][si] == man["body2"]).all(), "step %d" % s
        # nothing but solver_index changes, and only in live slots
        a, b = cps.copy(), recon.copy()
        live = np.zeros(len(cps), dtype=bool)
        live[spec.live_slots(m)] = True
        assert a[~live].tobytes() == b[~live].tobytes()
        a["solver_index"], b["solver_index"] = 0, 0
        assert a.tobytes() == b.tobytes()
    assert sensors_seen > 0


def test_state_transforms():
    f = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
    assert spec.spawn(f, 2).tolist() == [0, 1, 1, 0, 1, 0, 0]
    assert spec.remove(f, [1, 0, 1, 1, 0]).tolist() == [0, 1, 0]
    assert spec.set_state(3).tolist() == [0, 0, 0]
    assert spec.valid([0, 1, 2, 3, 0x80000000]).tolist() == [True, True, False, False, False]
