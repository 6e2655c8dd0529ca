"""Generate tests/golden/reference_*.npz from the REAL reference World / Collider / Solver.

Needs oracle/_ref/libphyx_ref_full_{strict,fast}.so, which `make -C oracle ref_full` builds from the reference's src/ as it lies
(with our no-op profiler header, oracle/ref_harness/profiler_off/).  The .npz files hold data only: inputs, the reference's
outputs and digests of them.  workers = 0 throughout (bit-identical run to run), and every step takes the
reference's parallel pair path (Collider::UpdatePairsParallel, full_harness.cpp PAIRS_PARALLEL): its serial path admits
duplicate pairs, which reference_lockstep.npz pins separately.

reference_{strict,fast}_<scene>.npz, per scene (2x50 stack, 10x100 stack, a 1k 'falling' scene) and per step s in {1,2,3}:
  solver inputs     bodies (raw 128-B records), contact points, contact joints (warm-start impulses included)
  ordering          joint_index after PrepareIndices for N = 1, 4, 8, island offsets / sizes (Multiple mode)
  per iteration     bodies + joints after k = 0..20 impulse iterations, re-run from the same state (_iteration_dumps says where)
  outputs           after the full solve (AVX2 / Single, 20 + 20), and the Multiple-mode solve's bodies; islandCount / islandMaxSize
  broadphase        sorted permutation (broadphaseSort[1]), BroadphaseEntry[], manifolds after UpdatePairs/PackManifolds

reference_lockstep.npz (strict build only): for every run of tests/reference_runs.py, the per-step SHA-256 digests of bodies,
manifolds, live contact points and joints; and the serial pair path's digests over the first steps of SERIAL_SCENE, the step at
which they first leave the parallel path's, and the pair the serial path holds twice there.

    make -C oracle ref_full && python tests/golden/make_reference_goldens.py
"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import binding as ob  # noqa: E402
from phyx_amd import scenes  # noqa: E402
import reference_runs as rr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = {"stack2x50": lambda: scenes.stack(2, 50), "stack10x100": lambda: scenes.stack(10, 100),
          "falling1k": lambda: scenes.falling(1000, width=400.0, ymax=600.0)}
DT = 1.0 / 60.0
SERIAL_STEPS = 12


def _contact_points(w):
    """The contact point array, its unowned slots (past a manifold's point_count) and padding bytes zeroed: the reference leaves
    them unwritten, and nothing reads them."""
    cp = np.zeros_like(w.contact_points())
    m = w.manifolds()
    first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    cp[live] = rr.live_contact_points(w)
    return cp


def _iteration_dumps(kind, name, step, n):
    """Which per-iteration dumps a fixture holds (kept under the fixtures' size budget): all of them at step 1 and on the 2x50
    stack; at steps 2 and 3 of the larger scenes the AVX2 path's full solve, and in the fast tier nothing past step 1."""
    if step == 1 or name == "stack2x50" and kind == "strict":
        return [0, 1, 2, 5, 10, 20]
    return [20] if kind == "strict" and n == 8 else []


def _world(kind, scene, history):
    """A reference world `history` full steps (AVX2 / Single, 20 + 20) into the scene, then everything before SolveJoints."""
    w = ob.RefWorld(kind)
    w.add_scene(scene)
    for _ in range(history):
        w.update(DT, ob.SOLVE_AVX2, ob.ISLAND_SINGLE, 20, 20)
    w.pre_solve(DT)
    return w


def dump(kind):
    for name, make in SCENES.items():
        out = {}
        scene = make()
        for k in ("px", "py", "angle", "sx", "sy", "static"):
            out["scene_" + k] = np.asarray(scene[k])
        w = ob.RefWorld(kind)
        w.add_scene(scene)
        for step in (1, 2, 3):
            w.pre_solve(DT)
            pre = "s%d_" % step
            out[pre + "in_bodies"], out[pre + "in_contact_points"], out[pre + "in_joints"] = w.bodies(), _contact_points(w), w.joints()
            out[pre + "manifolds"] = w.manifolds()
            out[pre + "broadphase_sorted"] = w.broadphase_sorted()
            out[pre + "broadphase_entries"] = w.broadphase_entries()
            # grouping + refresh + per-iteration dumps: fresh worlds replayed to the same state (workers = 0 is deterministic)
            for mode, n in ((ob.SOLVE_SCALAR, 1), (ob.SOLVE_SSE2, 4), (ob.SOLVE_AVX2, 8)):
                for iters in _iteration_dumps(kind, name, step, n):
                    w2 = _world(kind, scene, step - 1)
                    w2.solve(mode, ob.ISLAND_SINGLE, iters, 0 if iters < 20 else 20)
                    tag = pre + "n%d_it%d_" % (n, iters)
                    out[tag + "bodies"], out[tag + "joints"] = w2.bodies(), w2.joints()
                    if iters == 0:
                        out[pre + "n%d_joint_index" % n] = w2.joint_index()
            # Multiple island mode: partition and result
            w3 = _world(kind, scene, step - 1)
            w3.solve(ob.SOLVE_AVX2, ob.ISLAND_MULTIPLE, 20, 20)
            out[pre + "multiple_island_offset"] = w3.island_offset()
            out[pre + "multiple_island_size"] = w3.island_size()
            out[pre + "multiple_joint_index"] = w3.joint_index()
            out[pre + "multiple_island_stats"] = np.array(w3.island_stats(), dtype=np.int32)
            out[pre + "multiple_bodies"] = w3.bodies()
            # finish the step of the main world (AVX2 / Single, 20 + 20)
            w.solve(ob.SOLVE_AVX2, ob.ISLAND_SINGLE, 20, 20)
            w.integrate_position(DT)
            out[pre + "out_bodies"], out[pre + "out_joints"] = w.bodies(), w.joints()
        path = os.path.join(HERE, "reference_%s_%s.npz" % (kind, name))
        np.savez_compressed(path, **out)
        print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def dump_lockstep():
    out = {}
    for name, s, i in rr.RUNS:
        out[rr.run_key(name, s, i)] = rr.digests("strict", name, s, i)
    sm, im = rr.SERIAL_MODE
    serial = rr.digests("strict", rr.SERIAL_SCENE, sm, im, steps=SERIAL_STEPS, pairs=ob.PAIRS_SERIAL)
    parallel = out[rr.run_key(rr.SERIAL_SCENE, sm, im)][:SERIAL_STEPS]
    differs = np.flatnonzero((serial != parallel).any(axis=(1, 2)))
    assert len(differs), "the serial and parallel pair paths agree over %d steps" % SERIAL_STEPS
    first = int(differs[0]) + 1
    w = rr.make_world("strict", rr.SCENES[rr.SERIAL_SCENE][0](), ob.PAIRS_SERIAL)
    for _ in range(first):
        w.update(rr.DT, sm, im, rr.ITERS, rr.ITERS)
    m = w.manifolds()
    twice = [p for p, c in collections.Counter(zip(m["body1"].tolist(), m["body2"].tolist())).items() if c > 1]
    assert len(twice) == 1, twice
    out["serial_digests"] = serial
    out["serial_first_step"] = np.array(first, dtype=np.int32)        # 1-based: the state after this many steps
    out["serial_duplicate_pair"] = np.array(twice[0], dtype=np.int32)
    path = os.path.join(HERE, "reference_lockstep.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if any(ob.ref_full_lib(k) is None for k in ob.REF_KINDS):
        raise SystemExit("oracle/_ref/libphyx_ref_full_{strict,fast}.so are absent: run `make -C oracle ref_full` with the reference tree present")
    for kind in ob.REF_KINDS:
        dump(kind)
    dump_lockstep()
