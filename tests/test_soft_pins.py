"""Soft pins: what BASELINE.md §2 records of the COMPILED reference (the survey's probe runs, made when the reference could be
built with a stub profiler header) and the oracle reproduces today.  They were written before the reference's Solver.cpp / Collider.cpp /
World.cpp could be built here (tests/test_reference_*.py pin those now); they are not golden vectors and pin nothing formally:
they are bands around recorded behaviour of the real thing, and they fail if the restatement drifts away from it.

  * scalar vs AVX2 grouping on the 1k-box stack (cfg 1 scene): max |delta pos| after step 1 / 10 / 60 = 2.7e-2 / 0.50 / 81
    ("scalar vs AVX2, 1k stack"), band +-30 %;
  * the 200k-box stack (cfg 2 / cfg 3 scene): 1000-1003 islands of at most 404-500 joints at steps 3-8, 460 +-10 % on average (the
    probe's Multiple-mode row: "1003 islands, max 460 joints"), ~222-223k manifolds and ~440-446k joints around step 8-9 (its bodies / manifolds /
    joints column).
"""
import numpy as np

from oracle import binding as ob
from phyx_amd import scenes


def _positions(solve_mode, steps, marks):
    w = ob.OracleWorld(-200.0)
    w.add_scene(scenes.stack(10, 100))
    out = {}
    for s in range(1, steps + 1):
        w.update(1.0 / 60.0, solve_mode, ob.ISLAND_SINGLE, 20, 20)
        if s in marks:
            out[s] = w.bodies()["pos"].copy()
    return out


def test_scalar_vs_avx2_divergence_matches_the_reference_probe():
    recorded = {1: 2.7e-2, 10: 0.50, 60: 81.0}                      # BASELINE.md §2 (compiled reference, same scene, same settings)
    a = _positions(ob.SOLVE_SCALAR, 60, recorded)
    b = _positions(ob.SOLVE_AVX2, 60, recorded)
    for step, want in recorded.items():
        d = float(np.maximum(np.abs(a[step]["x"] - b[step]["x"]), np.abs(a[step]["y"] - b[step]["y"])).max())
        assert 0.7 * want <= d <= 1.3 * want, "step %d: scalar vs AVX2 max |delta pos| %.4g, the reference recorded %.4g" % (step, d, want)


def test_200k_stack_islands_and_contact_counts_match_the_reference_probe():
    w = ob.OracleWorld(-200.0)
    w.add_scene(scenes.stack(1000, 200))
    seen = {}
    for s in range(1, 10):
        w.update(1.0 / 60.0, ob.SOLVE_AVX2, ob.ISLAND_MULTIPLE, 20, 20)
        st = w.stats()
        seen[s] = (int(st.island_count), int(st.island_max_size), len(w.manifolds()), len(w.joints()))
    for s in range(3, 9):                                            # one island per column (+ the odd split), each a 200-box column's joints
        islands, biggest, _, _ = seen[s]
        assert 1000 <= islands <= 1003, (s, seen[s])
        assert 404 <= biggest <= 500, (s, seen[s])
    mean_biggest = np.mean([seen[s][1] for s in range(3, 10)])       # (the probe's "max 460 joints" is its average over steps 3-20)
    assert 0.9 * 460 <= mean_biggest <= 1.1 * 460, mean_biggest
    # the probe's counts column (200 001 bodies / 222-223k manifolds / 440-446k joints) is reached at steps 8-9 of a settling stack
    manifolds = [seen[s][2] for s in (8, 9)]
    joints = [seen[s][3] for s in (8, 9)]
    assert min(manifolds) <= 223_000 * 1.02 and max(manifolds) >= 222_000 * 0.98, manifolds
    assert min(joints) <= 446_000 * 1.02 and max(joints) >= 440_000 * 0.98, joints
