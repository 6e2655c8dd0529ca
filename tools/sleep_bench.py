"""What sleeping costs and saves (include/phyx_amd.h SLEEPING) in the settling 200k world: the cfg 2 world, stack(1000, 200), Single
Sloppy islands, 20 + 20 iterations, stepped with sleeping off, on, and with the pass running but nobody ever sleeping.

    python tools/sleep_bench.py [--nx 1000] [--ny 200] [--steps 110] [--lin 0.5] [--ang 0.05] [--time 0.5] [--only off|on|watch] [--import-from DIR]

Three worlds, stepped in turn, one synchronised World::Update at a time:
    off     sleeping never enabled: the parent commit's behaviour, the yardstick
    on      sleeping with the given parameters
    watch   sleeping with time_to_sleep = 1e30: the pass runs on a world that stays awake and so evolves exactly like `off`; the
            difference of the two is the pass's own time on a fully awake world, its most expensive state
Every step is timed twice: by the host clock between two synchronisations, and by two HIP events recorded on the world's stream
around the call.  One JSON line per world: the mean ms per step over steps 57-61 and 100-104 (both clocks), the step at which the
asleep count first reaches 90 % of the bodies, the schedule builds per 50 steps (phx_world_build_counts: from the manifolds + from
the joints), and for `watch` the pass's time per step (events, watch - off) over the same two windows.
--import-from takes phyx_amd from another tree (a build of the parent commit): only `off` exists there.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

WINDOWS = ((57, 61), (100, 104))


class Events:
    """two HIP events on a stream: the device time between them in ms"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, which, stream):
        assert self.hip.hipEventRecord(self.e[which], C.c_void_p(stream)) == 0

    def ms(self):
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        out = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(out), self.e[0], self.e[1]) == 0
        return out.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--ny", type=int, default=200)
    ap.add_argument("--steps", type=int, default=110)
    ap.add_argument("--lin", type=float, default=0.5)
    ap.add_argument("--ang", type=float, default=0.05)
    ap.add_argument("--time", type=float, default=0.5)
    ap.add_argument("--only", choices=("off", "on", "watch"), default=None)
    ap.add_argument("--import-from", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.import_from) if a.import_from else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import phyx_amd
    from phyx_amd import scenes
    cfg = phyx_amd.Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)
    dt = 1.0 / 60.0
    names = [a.only] if a.only else (["off"] if a.import_from else ["off", "on", "watch"])
    scene = scenes.stack(a.nx, a.ny)
    worlds = {}
    for name in names:
        w = phyx_amd.World(0, gravity=-200.0)
        w.add_scene(scene)
        if name == "on":
            w.set_sleeping(a.lin, a.ang, a.time)
        elif name == "watch":
            w.set_sleeping(a.lin, a.ang, 1e30)
        worlds[name] = w
    ev = Events()
    mobile = int((~scene["static"]).sum())
    wall = {n: [] for n in names}; dev = {n: [] for n in names}; asleep = {n: [] for n in names}; builds = {n: [] for n in names}
    for s in range(a.steps):
        for name, w in worlds.items():
            w.sync()
            stream = w.stream_ptr() or 0
            t0 = time.perf_counter()
            ev.record(0, stream)
            w.Update(dt, cfg)
            ev.record(1, stream)
            w.sync()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(ev.ms())
            asleep[name].append(w.sleep_counts()[0] if name != "off" and not a.import_from else 0)
            builds[name].append(sum(w.build_counts()))

    def window(v, lo, hi):
        return round(float(np.mean(v[lo:hi + 1])), 4) if len(v) > hi else None

    for name, w in worlds.items():
        out = {"world": name, "tree": os.path.dirname(os.path.abspath(phyx_amd.__file__)), "bodies": w.counts()[0], "manifolds": w.counts()[1], "joints": w.counts()[3],
               "steps": a.steps, "params": [a.lin, a.ang, a.time if name == "on" else (1e30 if name == "watch" else None)]}
        for lo, hi in WINDOWS:
            out["wall_ms_%d_%d" % (lo, hi)] = window(wall[name], lo, hi)
            out["event_ms_%d_%d" % (lo, hi)] = window(dev[name], lo, hi)
        reached = [s for s, n in enumerate(asleep[name]) if n >= 0.9 * mobile]
        out["asleep_90_percent_at_step"] = reached[0] if reached else None
        out["asleep_at_end"] = asleep[name][-1] if asleep[name] else 0
        out["schedule_builds_per_50_steps"] = [builds[name][min(k + 49, a.steps - 1)] - (builds[name][k - 1] if k else 0) for k in range(0, a.steps, 50)]
        if name == "watch" and "off" in worlds:
            for lo, hi in WINDOWS:
                if len(dev[name]) > hi:
                    out["pass_event_ms_%d_%d" % (lo, hi)] = round(float(np.mean(np.array(dev["watch"][lo:hi + 1]) - np.array(dev["off"][lo:hi + 1]))), 4)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
