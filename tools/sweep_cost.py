"""What continuous bodies cost, on one small pile in one process:

  plain                        this library: tools/polygon_cost.py's pen of `columns` x `rows` boxes dropped between two posts, no body
                               continuous: the world launches what the parent's launches;
  continuous_10 / _100 / _all  the same pen with its first 10, its first 100 or all of its bodies continuous (core radius 0.5, 2.5 inside
                               the boxes' inradius 3: clear of the 2 units a resting body lies inside what it rests on, so no body is
                               clamped and the worlds stay byte-identical): two more launches per step, the second one wave per continuous
                               body over all bodies;
  parent_a / parent_b          the plain pen on a library built at the parent commit (--parent-lib PATH), twice: two worlds of the same
                               bytes, whose difference is the run-to-run spread a difference has to exceed.

All worlds are warmed, then stepped in turns — `rounds` rounds of `chunk` steps each, the variants alternating — and a step is timed by
the host clock around phx_world_update + phx_world_synchronize.  Per variant: the median step, the 10th and 90th percentile and the
spread of its per-round medians; for the continuous pens also the pass kernel's own time between two HIP events
(phx_world_sweep_timing), its median over the timed steps, and the clamps the pile made (none is expected: the pens are byte-identical
worlds and the figures compare launches, not different piles).  One condition is checked: the plain pen against the
parent's, within the larger of the parent's own spread and the distance between its two runs.

Prints one JSON line.  There is no fallback: without a device the world cannot be created and the tool fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phyx_amd                                                    # noqa: E402
from phyx_amd import Configuration                                 # noqa: E402
from capsule_cost import BOX, DT, Raw                              # noqa: E402


class Continuous(Raw):
    """The pen as boxes, its first `count` bodies behind the floor and the posts continuous."""

    def __init__(self, lib, count, columns, rows, hx, hy):
        Raw.__init__(self, lib, BOX, columns, rows, hx, hy)
        vp, i32 = C.c_void_p, C.c_int32
        lib.phx_world_set_continuous.restype, lib.phx_world_set_continuous.argtypes = C.c_int, [vp, vp, vp, i32]
        lib.phx_world_sweep_timing.restype, lib.phx_world_sweep_timing.argtypes = C.c_int, [vp, i32, C.POINTER(C.c_double)]
        lib.phx_world_sweep_counts.restype, lib.phx_world_sweep_counts.argtypes = C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        idx = np.arange(3, 3 + count, dtype=np.int32)
        radii = np.full(count, min(hx, hy) - 2.5, dtype=np.float32)
        self.ok(lib.phx_world_set_continuous(self.h, idx.ctypes.data, radii.ctypes.data, count))
        self.ok(lib.phx_world_sweep_timing(self.h, 1, None))
        self.kernel_ms = []

    def pass_ms(self):
        ms = C.c_double(0.0)
        self.ok(self.L.phx_world_sweep_timing(self.h, 1, C.byref(ms)))
        return ms.value

    def sweep_counts(self):
        passes, clamps = C.c_int64(0), C.c_int64(0)
        self.ok(self.L.phx_world_sweep_counts(self.h, C.byref(passes), C.byref(clamps)))
        return passes.value, clamps.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libphyx_amd.so built at the parent commit")
    ap.add_argument("--warmup", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--columns", type=int, default=40)
    ap.add_argument("--rows", type=int, default=25)
    args = ap.parse_args()
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)._c()      # bench.py's cfg 2
    here = C.CDLL(os.path.join(ROOT, "phyx_amd", "libphyx_amd.so"))
    hx, hy = 6.0, 3.0
    size = (args.columns, args.rows, hx, hy)
    n = args.columns * args.rows
    worlds = {"plain": Raw(here, BOX, *size)}
    for count in sorted({min(10, n), min(100, n), n}):
        worlds["continuous_all" if count == n else "continuous_%d" % count] = Continuous(here, count, *size)
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for run in "ab":
            worlds["parent_" + run] = Raw(parent, BOX, *size)
    names = list(worlds)

    def step(name):
        w = worlds[name]
        st = w.L.phx_world_update(w.h, DT, C.byref(cfg))
        st = st or w.L.phx_world_synchronize(w.h)
        if st:
            raise RuntimeError("%s: status %d: %s" % (name, st, w.L.phx_last_error().decode()))

    for name in names:
        for _ in range(args.warmup):
            step(name)
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:                                         # the variants alternate: drift of the machine touches all alike
            chunk = []
            for _ in range(args.chunk):
                t0 = time.perf_counter()
                step(name)
                chunk.append(time.perf_counter() - t0)
                if isinstance(worlds[name], Continuous):
                    worlds[name].kernel_ms.append(worlds[name].pass_ms())
            times[name].append(chunk)
    out = {"pile": "%d x %d boxes {6, 3}" % (args.columns, args.rows), "warmup": args.warmup, "rounds": args.rounds, "chunk": args.chunk, "ms": {},
           "manifolds": {name: worlds[name].manifolds() for name in names}, "k_sweep_bodies_ms": {}, "sweep_counts": {}}
    for name in names:
        t = 1e3 * np.array(times[name])
        medians = np.median(t, axis=1)
        out["ms"][name] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4),
                           "round_spread": round(float(medians.max() - medians.min()), 4)}
        if isinstance(worlds[name], Continuous):
            k = np.array(worlds[name].kernel_ms)
            out["k_sweep_bodies_ms"][name] = {"median": round(float(np.median(k)), 5), "p90": round(float(np.percentile(k, 90)), 5)}
            out["sweep_counts"][name] = worlds[name].sweep_counts()
            out[name + "_minus_plain_ms"] = round(out["ms"][name]["median"] - float(np.median(1e3 * np.array(times["plain"]))), 4)
    ok = True
    if args.parent_lib:
        a, b, c = (out["ms"][k]["median"] for k in ("parent_a", "parent_b", "plain"))
        spread = max(abs(a - b), out["ms"]["parent_a"]["round_spread"], out["ms"]["parent_b"]["round_spread"])
        ok = bool(abs(c - 0.5 * (a + b)) <= spread)
        out["plain_vs_parent"] = {"minus_parent_ms": round(c - 0.5 * (a + b), 4), "parent_spread_ms": round(spread, 4), "within": ok}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
