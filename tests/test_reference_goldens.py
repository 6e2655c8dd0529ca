"""Pins of the oracle against fixtures dumped from the REAL reference (tests/golden/make_reference_goldens.py).

The fixtures are data only, committed, and made from oracle/_ref/libphyx_ref_full_{strict,fast}.so (the reference's World.cpp,
Solver.cpp and Collider.cpp built as they lie, oracle/Makefile `ref_full`), every step on the reference's parallel pair path.
These tests need nothing but the fixtures and the oracle.

Tiers:
  * STRICT build (-fno-fast-math -ffp-contract=off): bit for bit, stage by stage: bodies, joints, broadphase entries, live contact
    points, the sorted order, manifolds, PrepareIndices for N = 1 / 4 / 8, the per-iteration dumps, the Multiple-mode partition and
    bodies, and the outputs of the step.
  * FAST build (the reference's own flags): integer stages (sort permutation, manifolds, PrepareIndices, island partition) exact;
    velocities after 0-1 iterations within 1e-5, after more within VEL_TOL = 1e-3; positions within POS_ULPS units in the last place
    of max(|x|, 1), plus the dt * VEL_TOL that a velocity inside its bound moves a body in one step.  (A plain absolute bound such
    as 1e-4 goes below float resolution once |x| >= 256: 1e-4 is under 4 ulps at |x| = 460.)
The strict tier's byte equality on the same fields is strictly stronger than the fast tier's bounds."""
import glob
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "reference_strict_*.npz")) +
                  glob.glob(os.path.join(HERE, "golden", "reference_fast_*.npz")))
POS_ULPS = 8
VEL_TOL = 1e-3
DT = 1.0 / 60.0


def test_the_fixtures_are_committed():
    names = sorted(os.path.basename(p) for p in FIXTURES)
    assert names == sorted("reference_%s_%s.npz" % (k, s) for k in ("strict", "fast") for s in ("stack2x50", "stack10x100", "falling1k"))


def _world_at(oracle, g, step):
    scene = {k: g["scene_" + k] for k in ("px", "py", "angle", "sx", "sy", "static")}
    w = oracle.OracleWorld(-200.0)
    w.add_scene(scene)
    for _ in range(step - 1):
        w.update(contact_iters=20, penetration_iters=20, solve_mode=oracle.SOLVE_AVX2, island_mode=oracle.ISLAND_SINGLE)
    w.pre_solve(DT)
    return w


def _live_points(cps, manifolds):
    first, count = manifolds["point_index"].astype(np.int64), manifolds["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    cp = cps[live].copy()
    cp["pad"] = 0
    return cp


def _pos_close(got, want, what):
    for f in ("x", "y"):
        a, b = got["pos"][f], want["pos"][f]
        bound = POS_ULPS * np.spacing(np.maximum(np.abs(b), np.float32(1.0))) + DT * VEL_TOL
        worst = np.argmax(np.abs(a - b) - bound) if len(a) else 0
        assert (np.abs(a - b) <= bound).all(), "%s pos.%s: %r against %r" % (what, f, a[worst], b[worst])


def _vel_close(got, want, tol, what):
    for f in ("x", "y"):
        assert np.abs(got["velocity"][f] - want["velocity"][f]).max(initial=0.0) <= tol, what
    assert np.abs(got["angular_velocity"] - want["angular_velocity"]).max(initial=0.0) <= tol, what


def _multiple_islands_equal(order, g, pre):
    """GatherIslands (ref: Solver.cpp:285-453): the partition, and each island's joints in order.  The padding slots of the aligned
    joint_index are left unwritten by the reference, so only [offset, offset + size) of every island is compared; island_offset and
    island_size are sized for the islands before coalescing, and only the first islandCount entries are written."""
    off, size = g[pre + "multiple_island_offset"], g[pre + "multiple_island_size"]
    ref = g[pre + "multiple_joint_index"]
    count = int(g[pre + "multiple_island_stats"][0])
    assert 0 < count <= min(len(off), len(size))
    assert int(off[count - 1]) + int(size[count - 1]) <= len(ref) <= len(order)
    for i in range(count):
        a, n = int(off[i]), int(size[i])
        assert order[a:a + n].tolist() == ref[a:a + n].tolist(), "island %d (offset %d, size %d)" % (i, a, n)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_oracle_matches_the_reference(oracle, path):
    g = np.load(path)
    strict = "_strict_" in os.path.basename(path)
    for step in (1, 2, 3):
        pre = "s%d_" % step
        w = _world_at(oracle, g, step)
        b, cp, j, m = w.bodies(), w.contact_points(), w.joints(), w.manifolds()
        # integer / byte stages: exact under both builds
        assert m.tobytes() == g[pre + "manifolds"].tobytes(), "step %d" % step
        _, srt, ent = oracle.broadphase_build(b)
        assert srt["index"].tolist() == g[pre + "broadphase_sorted"]["index"].tolist()
        assert j[["contact_point_index", "body1", "body2"]].tolist() == g[pre + "in_joints"][["contact_point_index", "body1", "body2"]].tolist()
        if strict:
            assert b.tobytes() == g[pre + "in_bodies"].tobytes() and j.tobytes() == g[pre + "in_joints"].tobytes()
            assert ent.tobytes() == g[pre + "broadphase_entries"].tobytes()
            assert srt.tobytes() == g[pre + "broadphase_sorted"].tobytes()
            assert _live_points(cp, m).tobytes() == _live_points(g[pre + "in_contact_points"], m).tobytes()
        else:
            _pos_close(b, g[pre + "in_bodies"], "step %d in_bodies" % step)
        for mode, n in ((oracle.SOLVE_SCALAR, 1), (oracle.SOLVE_SSE2, 4), (oracle.SOLVE_AVX2, 8)):
            if step == 1:
                assert pre + "n%d_it20_bodies" % n in g
            for iters in (0, 1, 2, 5, 10, 20):
                key = pre + "n%d_it%d_bodies" % (n, iters)
                if key not in g:
                    continue
                bb, jj = g[pre + "in_bodies"].copy(), g[pre + "in_joints"].copy()        # the REFERENCE's inputs: stage-level parity
                order, st = oracle.solver_solve(bb, g[pre + "in_contact_points"], jj, mode, oracle.ISLAND_SINGLE, iters, 0 if iters < 20 else 20)
                if iters == 0:
                    assert order[:len(jj)].tolist() == g[pre + "n%d_joint_index" % n].tolist()       # PrepareIndices: exact
                if strict:
                    assert bb.tobytes() == g[key].tobytes() and jj.tobytes() == g[pre + "n%d_it%d_joints" % (n, iters)].tobytes(), key
                else:
                    _vel_close(bb, g[key], 1e-5 if iters <= 1 else VEL_TOL, key)
        # Multiple island mode, from the reference's inputs
        bb, jj = g[pre + "in_bodies"].copy(), g[pre + "in_joints"].copy()
        order, st = oracle.solver_solve(bb, g[pre + "in_contact_points"], jj, oracle.SOLVE_AVX2, oracle.ISLAND_MULTIPLE, 20, 20)
        assert [st.island_count, st.island_max_size] == g[pre + "multiple_island_stats"].tolist()            # GatherIslands: exact
        _multiple_islands_equal(order, g, pre)
        if strict:
            assert bb.tobytes() == g[pre + "multiple_bodies"].tobytes()
        else:
            _vel_close(bb, g[pre + "multiple_bodies"], VEL_TOL, "step %d multiple_bodies" % step)
        # the rest of the oracle world's own step (AVX2 / Single, 20 + 20)
        w.solve_and_integrate(DT, oracle.SOLVE_AVX2, oracle.ISLAND_SINGLE, 20, 20)
        ob, oj = w.bodies(), w.joints()
        if strict:
            assert ob.tobytes() == g[pre + "out_bodies"].tobytes() and oj.tobytes() == g[pre + "out_joints"].tobytes()
        else:
            _pos_close(ob, g[pre + "out_bodies"], "step %d out_bodies" % step)
            _vel_close(ob, g[pre + "out_bodies"], VEL_TOL, "step %d out_bodies" % step)
