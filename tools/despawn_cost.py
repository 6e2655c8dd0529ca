"""Wall time of removing bodies from the cfg 2 world (stack(1000, 200), 200 001 bodies), three ways:

  killplane  remove_outside(box) with the box's top lowered by one row of boxes per call: the device tests the AABBs (phx_world_remove_outside);
  random     remove_bodies of 1 % of the bodies, drawn at random (phx_world_remove_bodies);
  roundtrip  the same 1 % through the full state: state(), the filter on the host (tests/removal_spec.py), set_state(...).

`python tools/despawn_cost.py [--warmup W] [--calls K]` runs each loop in a child process of its own under a time limit, stops at the
first one that fails, and prints one JSON line: the median wall time per call (the call, its readback and a stream synchronisation;
the step between two calls is not timed).  Every loop starts from a fresh world warmed by W plain steps.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ("killplane", "random", "roundtrip")


def run_loop(kind, warmup, calls):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import phyx_amd
    import removal_spec
    from phyx_amd import Configuration, scenes
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)      # bench.py's cfg 2
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scenes.stack(1000, 200))
    for _ in range(warmup):
        w.Update(1.0 / 60.0, cfg)
    w.sync()
    rng = np.random.default_rng(1)
    top = float(w.bodies["aabb_max"]["y"].max())
    times, removed = [], 0
    for k in range(calls):
        n = w.counts()[0]
        pick = rng.choice(n, size=max(1, n // 100), replace=False).astype(np.int32)
        t0 = time.perf_counter()
        if kind == "killplane":
            gone, _ = w.remove_outside((-1e5, -1e5, 1e5, top - 10.0 * (k + 1)))
        elif kind == "random":
            w.remove_bodies(pick)
            gone = len(pick)
        else:
            state = w.state()
            (b, m, cp, j), _ = removal_spec.filter(state, pick)
            w.set_state(b, m, cp, j)
            gone = len(pick)
        w.sync()
        times.append(time.perf_counter() - t0)
        removed += gone
        w.Update(1.0 / 60.0, cfg)
        w.sync()
    print(json.dumps({"loop": kind, "ms_per_call": 1e3 * float(np.median(times)), "min_ms": 1e3 * min(times), "calls": calls,
                      "removed": removed, "bodies": int(w.counts()[0])}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds each loop's child process may take")
    ap.add_argument("--loop", choices=LOOPS, help=argparse.SUPPRESS)                  # (the child's side)
    args = ap.parse_args()
    if args.loop:
        run_loop(args.loop, args.warmup, args.calls)
        return 0
    out = {"scene": "stack(1000, 200)", "warmup": args.warmup, "calls": args.calls}
    for kind in LOOPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop", kind, "--warmup", str(args.warmup), "--calls", str(args.calls)],
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            out[kind] = "timed out after %.0f s" % args.timeout
            break
        if r.returncode != 0:
            out[kind] = "exit %d: %s" % (r.returncode, r.stderr[-400:])
            break
        out[kind] = json.loads(r.stdout.strip().splitlines()[-1])["ms_per_call"]
    print(json.dumps(out))
    return 0 if all(isinstance(out.get(k), float) for k in LOOPS) else 1


if __name__ == "__main__":
    sys.exit(main())
