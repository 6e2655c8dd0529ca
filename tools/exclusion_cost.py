"""What collision exclusions cost on the cfg 2 world (stack(1000, 200), bench.py's configuration).  Every timing runs in a process of
its own: without --variant the tool starts itself once per variant, one child after the other, and gathers their lines.

  empty     this library, no exclusion set: the plain sweep kernels (the step a world pays that never heard of exclusions);
  corner    1 000 excluded pairs among the first 2 000 boxes (ten columns of one corner), body i with body i + 1000 — the realistic
            case: a mechanism in a large world.  Almost every sweep row reads a zero word and makes no probe;
  all       every box in one pair, (i, i + n / 2): every row probes once per y-overlapping candidate that passed the filter.

No excluded pair ever overlaps (the partners are five columns resp. half the world apart), so every variant computes the trajectory
of `empty`, byte for byte — checked by a digest of the bodies — and the differences are the exclusion test alone.  A step is timed
by the host clock around phx_world_update + phx_world_synchronize, after `warmup` steps; per variant: the median step, the 10th and
90th percentile.  The sweep kernels' own time comes from a kernel trace in a run of its own:
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/exclusion_cost.py --variant all`.

Prints one JSON line.  There is no fallback: without a device the world cannot be created and the tool fails."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 1.0 / 60.0
G = -200.0
VARIANTS = ("empty", "corner", "all")


def pairs_of(variant, boxes):
    if variant == "corner":
        i = np.arange(1, 1001)
        return np.stack([i, i + 1000], axis=1).astype(np.int32)
    if variant == "all":
        i = np.arange(1, boxes // 2 + 1)
        return np.stack([i, i + boxes // 2], axis=1).astype(np.int32)
    return np.zeros((0, 2), dtype=np.int32)


def one(args):
    import phyx_amd
    from phyx_amd import Configuration, scenes
    scene = scenes.stack(args.columns, args.rows)
    boxes = len(scene["px"]) - 1
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)._c()      # bench.py's cfg 2
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scene)
    pairs = pairs_of(args.variant, boxes)
    t0 = time.perf_counter()
    dropped = w.add_collision_exclusions(pairs)
    add_ms = 1e3 * (time.perf_counter() - t0)

    def step():
        phyx_amd.api.check(w.L.phx_world_update(w.h, DT, C.byref(cfg)))
        phyx_amd.api.check(w.L.phx_world_synchronize(w.h))

    for _ in range(args.warmup):
        step()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step()
        t.append(1e3 * (time.perf_counter() - t0))
    t = np.array(t)
    stats = w.collider.stats()
    out = {"variant": args.variant, "scene": "stack(%d, %d)" % (args.columns, args.rows), "bodies": boxes + 1, "pairs": int(len(pairs)),
           "dropped": int(dropped), "add_ms": round(add_ms, 3), "warmup": args.warmup, "steps": args.steps,
           "ms": {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4)},
           "overlapping_pairs_last_step": int(stats.overlapping_pairs), "set_size": int(stats.set_size),
           "bodies_sha1": hashlib.sha1(w.bodies.tobytes()).hexdigest()}
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", choices=VARIANTS, help="measure this variant in this process (default: one child process per variant)")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--columns", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=1, help="children per variant, the variants alternating")
    args = ap.parse_args()
    if args.variant:
        return one(args)
    runs = []
    for _ in range(args.repeats):
        for v in VARIANTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--warmup", str(args.warmup), "--steps", str(args.steps),
                                "--columns", str(args.columns), "--rows", str(args.rows)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"runs": runs, "same_trajectory": len({r["bodies_sha1"] for r in runs}) == 1}
    for v in VARIANTS:
        m = [r["ms"]["median"] for r in runs if r["variant"] == v]
        out[v + "_median_ms"] = round(float(np.median(m)), 4)
        out[v + "_spread_ms"] = round(float(max(m) - min(m)), 4)
    print(json.dumps(out))
    return 0 if out["same_trajectory"] else 1


if __name__ == "__main__":
    sys.exit(main())
