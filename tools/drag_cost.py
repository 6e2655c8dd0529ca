"""Per-step cost of the reference's demo drag (ref: main.cpp:337-349) on the cfg 2 world, three ways:

  plain      World::Update alone;
  drag       body_states([1]) + add_accelerations([1], a) + Update — the edit calls (phx_world_get_body_states / add_accelerations);
  roundtrip  the same drag through the full state: state() (get_bodies + the contact cache), `acceleration += a` on the host,
             set_state(...), Update.

`python tools/drag_cost.py [--warmup W] [--steps K]` runs each loop in a child process of its own under a time limit, stops at the
first one that fails, and prints one JSON line: the median wall time per step (a step = its calls + a stream synchronisation) of each.
Every loop starts from a fresh world warmed by W plain steps, so the three time the same stretch of the simulation.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ("plain", "drag", "roundtrip")


def run_loop(kind, warmup, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import phyx_amd
    from phyx_amd import Configuration, scenes
    g = -200.0
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)      # bench.py's cfg 2
    w = phyx_amd.World(0, gravity=g)
    w.add_scene(scenes.stack(1000, 200))
    for _ in range(warmup):
        w.Update(1.0 / 60.0, cfg)
    w.sync()

    def accel(rec, target):
        pos = np.array([rec["pos"]["x"], rec["pos"]["y"]], dtype=np.float32)
        vel = np.array([rec["velocity"]["x"], rec["velocity"]["y"]], dtype=np.float32)
        a = np.array([0.0, -g], dtype=np.float32)
        a += ((target - pos) * np.float32(50.0) - vel) * np.float32(5.0)
        return a

    target = None
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        if kind == "drag":
            rec = w.body_states([1])[0]
            if target is None:
                target = np.array([rec["pos"]["x"], rec["pos"]["y"] + 20.0], dtype=np.float32)
            a = accel(rec, target)
            w.add_accelerations([1], np.array([[a[0], a[1], 0.0]], dtype=np.float32))
        elif kind == "roundtrip":
            b, m, cp, j = w.state()
            if target is None:
                target = np.array([b["pos"]["x"][1], b["pos"]["y"][1] + 20.0], dtype=np.float32)
            a = accel(b[1], target)
            b["acceleration"]["x"][1] += a[0]
            b["acceleration"]["y"][1] += a[1]
            w.set_state(b, m, cp, j)
        w.Update(1.0 / 60.0, cfg)
        w.sync()
        times.append(time.perf_counter() - t0)
    print(json.dumps({"loop": kind, "ms_per_step": 1e3 * float(np.median(times)), "min_ms": 1e3 * min(times), "steps": steps,
                      "bodies": int(w.counts()[0])}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds each loop's child process may take")
    ap.add_argument("--loop", choices=LOOPS, help=argparse.SUPPRESS)                  # (the child's side)
    args = ap.parse_args()
    if args.loop:
        run_loop(args.loop, args.warmup, args.steps)
        return 0
    out = {"scene": "stack(1000, 200)", "warmup": args.warmup}
    for kind in LOOPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop", kind, "--warmup", str(args.warmup), "--steps", str(args.steps)],
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            out[kind] = "timed out after %.0f s" % args.timeout
            break
        if r.returncode != 0:
            out[kind] = "exit %d: %s" % (r.returncode, r.stderr[-400:])
            break
        out[kind] = json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]
    print(json.dumps(out))
    return 0 if all(isinstance(out.get(k), float) for k in LOOPS) else 1


if __name__ == "__main__":
    sys.exit(main())
