"""What round bodies cost on the cfg 2 world (stack(1000, 200), bench.py's configuration), in one process:

  parent    the steady step of a library built at the parent commit (--parent-lib PATH; left out when none is given);
  none      this library, no shape column: UpdateManifolds' box/box instantiation, the parent's path;
  boxes     this library with the column active and every body a box: the instantiation that reads the kinds, one 4-byte gather per body
            of a manifold, taking the box/box routine every time (the same trajectory as `none`, checked);
  circles   ... with half of the dynamic bodies turned into circles of radius 5 (every other body; their masses set to a disc's).

All worlds are warmed, then stepped in turns — `rounds` rounds of `chunk` steps each, the variants alternating — and a step is timed by
the host clock around phx_world_update + phx_world_synchronize.  Per variant: the median step, the 10th and 90th percentile, and the
spread of its per-round medians (max - min), which is the run-to-run noise a difference has to exceed.  Then every world runs
`phase_steps` more steps with per-phase timing on (one stream synchronisation per phase): the UpdateManifolds phase is the
narrowphase kernel with its launch, over all manifolds (with the phases timed one by one no manifold is updated under the
broadphase's round trip).  One condition is checked: `none` equals `parent` within the parent's own spread.

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
import phyx_amd                                                    # noqa: E402
from phyx_amd import Configuration, scenes                         # noqa: E402
from phyx_amd._lib import Config                                   # noqa: E402

DT = 1.0 / 60.0
G = -200.0
UPDATE_MANIFOLDS = 3                                               # World.PHASES


class Raw:
    """The few calls the loop needs, on any build of the library (the parent's knows no shapes)."""

    def __init__(self, lib, scene):
        self.L = lib
        vp, f32, i32 = C.c_void_p, C.c_float, C.c_int32
        for name, res, args in (("phx_world_create", C.c_int, [C.POINTER(vp), C.c_int]), ("phx_world_destroy", None, [vp]),
                                ("phx_world_add_body", C.c_int, [vp, f32, f32, f32, f32, f32]), ("phx_world_set_body_static", C.c_int, [vp, i32]),
                                ("phx_world_set_gravity", C.c_int, [vp, f32]), ("phx_world_update", C.c_int, [vp, f32, C.POINTER(Config)]),
                                ("phx_world_synchronize", C.c_int, [vp]), ("phx_world_set_phase_timing", C.c_int, [vp, i32]),
                                ("phx_world_get_phase_ms", C.c_int, [vp, C.POINTER(C.c_double)]), ("phx_last_error", C.c_char_p, [])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.h = vp()
        self.ok(lib.phx_world_create(C.byref(self.h), 0))
        self.ok(lib.phx_world_set_gravity(self.h, G))
        for k in range(len(scene["px"])):
            i = lib.phx_world_add_body(self.h, float(scene["px"][k]), float(scene["py"][k]), float(scene["angle"][k]), float(scene["sx"][k]), float(scene["sy"][k]))
            self.ok(i)
            if scene["static"][k]:
                self.ok(lib.phx_world_set_body_static(self.h, i))

    def ok(self, st):
        if st < 0:
            raise RuntimeError("status %d: %s" % (st, self.L.phx_last_error().decode()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libphyx_amd.so built at the parent commit")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--phase-steps", type=int, default=20)
    ap.add_argument("--columns", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--only", help="comma-separated variants (default: all)")
    args = ap.parse_args()
    scene = scenes.stack(args.columns, args.rows)
    n = len(scene["px"])
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)._c()      # bench.py's cfg 2

    names = ["none", "boxes", "circles"]
    if args.parent_lib:
        names.insert(0, "parent")
    if args.only:
        names = [v for v in names if v in args.only.split(",")]
    worlds, handles = {}, {}
    dynamic = np.flatnonzero(~np.asarray(scene["static"], dtype=bool)).astype(np.int32)
    for name in names:
        if name == "parent":
            worlds[name] = Raw(C.CDLL(os.path.abspath(args.parent_lib)), scene)
            handles[name] = (worlds[name].L, worlds[name].h)
            continue
        w = phyx_amd.World(0, gravity=G)
        w.add_scene(scene)
        if name == "boxes":                                            # the column exists, every body is a box again
            size = (float(scene["sx"][dynamic[0]]), float(scene["sy"][dynamic[0]]))
            w.set_shapes(dynamic[:1], phyx_amd.SHAPE_CIRCLE, size[0])
            w.set_shapes(dynamic[:1], phyx_amd.SHAPE_BOX, size[0], size[1])
        if name == "circles":
            half = dynamic[::2]
            w.set_shapes(half, phyx_amd.SHAPE_CIRCLE, 5.0)
            w.set_inverse_masses(half, np.repeat(phyx_amd.circle_inverse_masses(5.0), len(half), axis=0))
        worlds[name] = w
        handles[name] = (w.L, w.h)

    def step(name):
        lib, h = handles[name]
        st = lib.phx_world_update(h, DT, C.byref(cfg))
        st = st or lib.phx_world_synchronize(h)
        if st:
            raise RuntimeError("%s: status %d: %s" % (name, st, lib.phx_last_error().decode()))

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
            times[name].append(chunk)

    out = {"scene": "stack(%d, %d)" % (args.columns, args.rows), "bodies": n, "warmup": args.warmup, "rounds": args.rounds, "chunk": args.chunk, "ms": {},
           "update_manifolds_phase_ms": {}}
    for name in names:
        t = 1e3 * np.array(times[name])
        medians = np.median(t, axis=1)
        out["ms"][name] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4),
                           "round_spread": round(float(medians.max() - medians.min()), 4)}
    if "none" in names and "boxes" in names:                       # (before the phase-timed steps: the same number of steps behind both)
        out["boxes_same_trajectory"] = worlds["none"].bodies.tobytes() == worlds["boxes"].bodies.tobytes()
    for name in names:
        lib, h = handles[name]
        lib.phx_world_set_phase_timing(h, 1)
        phase, ms = [], (C.c_double * 8)()
        for _ in range(args.phase_steps):
            step(name)
            lib.phx_world_get_phase_ms(h, ms)
            phase.append(ms[UPDATE_MANIFOLDS])
        lib.phx_world_set_phase_timing(h, 0)
        out["update_manifolds_phase_ms"][name] = {"median": round(float(np.median(phase)), 4), "p10": round(float(np.percentile(phase, 10)), 4),
                                                  "p90": round(float(np.percentile(phase, 90)), 4)}
    out["manifolds"] = {name: int(worlds[name].counts()[1]) for name in names if name != "parent"}
    if "parent" in names and "none" in names:
        diff = out["ms"]["none"]["median"] - out["ms"]["parent"]["median"]
        out["none_minus_parent_ms"] = round(diff, 4)
        out["none_within_parent_spread"] = bool(abs(diff) <= out["ms"]["parent"]["round_spread"])
    print(json.dumps(out))
    return 0 if out.get("none_within_parent_spread", True) and out.get("boxes_same_trajectory", True) else 1


if __name__ == "__main__":
    sys.exit(main())
