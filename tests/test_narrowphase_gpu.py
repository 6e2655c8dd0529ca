"""The device's narrowphase (phyx_amd/csrc/narrowphase.h, k_update_manifolds, the manifold pack, the joint match) on the directed
corpus of tests/narrowphase_corpus.py, whose reach over every arm tests/test_narrowphase_cpu.py proves on the CPU: one device World
and one oracle World walked through the corpus's phases in lockstep, every byte compared after every step; and a twin against the
reference's own World where its library is present."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration
from oracle import binding as ob
import narrowphase_corpus as nc
import reference_runs as rr
import spawn_lockstep
from helpers import oracle_set_pose, oracle_set_velocity

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 4, 4)


def _device_world(cs):
    """Built by add_scene from phase 1.  phx_world_add_body refuses a half size of 0 (such a box has no mass), so a world that holds
    one is loaded with the records the oracle's constructor gives the same scene (phx_world_set_state takes records as they are)."""
    pw = phyx_amd.World(0, gravity=0.0)
    sc = nc.scene(cs)
    if min(sc["sx"].min(), sc["sy"].min()) > 0:
        pw.add_scene(sc)
    else:
        ow = ob.OracleWorld(0.0)
        ow.add_scene(sc)
        none = lambda dtype: np.zeros(0, dtype=dtype)
        pw.set_state(ow.bodies(), none(ob.manifold_dtype), none(ob.contact_point_dtype), none(ob.joint_dtype))
    return pw


def _pose_device(pw, frames):
    idx = np.arange(len(frames), dtype=np.int32)
    pw.set_poses(idx, frames)
    pw.set_velocities(idx, np.zeros((len(frames), 3), dtype=np.float32))


@pytest.mark.parametrize("count", [1, 2, 127, 128, 129, None])
def test_corpus_lockstep_with_the_oracle(oracle, built_lib, count):
    cs = nc.cases()[:count]
    pw = _device_world(cs)
    ow = oracle.OracleWorld(0.0)
    ow.add_scene(nc.scene(cs))
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    contacts = 0
    for p in range(nc.MAX_PHASES):
        if p:
            frames = nc.phase_frames(cs, p)
            _pose_device(pw, frames)
            for i, f in enumerate(frames):
                oracle_set_pose(oracle, ow, i, f)
                oracle_set_velocity(ow, i, (0.0, 0.0, 0.0))
            assert pw.bodies.tobytes() == ow.bodies().tobytes(), "bodies differ before phase %d" % p
        spawn_lockstep.step(oracle, pw, ow, CFG, DT)
        spawn_lockstep.compare(pw, ow, p)
        assert pw.debug_counters()["dropped_points"] == oracle.lib().phxo_world_point_overflows(ow.h) == 0
        contacts += len(ow.joints())
    assert contacts > 0


@pytest.mark.skipif(not ob.ref_full_can_pose("strict"), reason=ob.REF_POSE_SKIP)
def test_corpus_against_the_reference_world(built_lib):
    """No oracle in the loop: manifolds, live contact points and joint topology against the reference's own Collider and
    RefreshContactJoints, every phase (the solve is order dependent and is pinned through the oracle above)."""
    cs = nc.cases()
    pw = _device_world(cs)
    rw = ob.RefWorld("strict", 0.0, ob.PAIRS_PARALLEL)
    rw.add_scene(nc.scene(cs))
    contacts = 0
    for p in range(nc.MAX_PHASES):
        if p:
            frames = nc.phase_frames(cs, p)
            _pose_device(pw, frames)
            for i, f in enumerate(frames):
                rw.set_pose(i, f)
                rw.set_velocity(i, (0.0, 0.0, 0.0))
        rw.update(DT, ob.SOLVE_AVX2, ob.ISLAND_SINGLE, 4, 4)
        pw.Update(DT, CFG)
        m = rw.manifolds()
        assert pw.counts()[1:] == (len(m), len(rw.contact_points()), len(rw.joints())), "phase %d" % p
        assert pw.manifolds.tobytes() == m.tobytes(), "manifolds differ after phase %d" % p
        dm = pw.manifolds
        first, count = dm["point_index"].astype(np.int64), dm["point_count"].astype(np.int64)
        live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
        cp = pw.contactPoints[live].copy()
        cp["pad"] = 0
        assert cp.tobytes() == rr.live_contact_points(rw).tobytes(), "contact points differ after phase %d" % p
        dj, rj = pw.contactJoints, rw.joints()
        for f in ("contact_point_index", "body1", "body2"):
            assert (dj[f] == rj[f]).all(), "joint %s differ after phase %d" % (f, p)
        contacts += len(rj)
    assert contacts > 0
