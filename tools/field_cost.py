"""What force fields cost on the cfg 2 world (stack(1000, 200), bench.py's configuration), in one process:

  parent        the steady step of a library built at the parent commit (--parent-lib PATH; left out when none is given);
  none          this library, no field list;
  uniform-K     this library with K = 1, 16, 256 ALL-region UNIFORM fields (the cheapest record);
  radial-K      ... with K disc-region RADIAL fields with a falloff whose disc holds the whole stack (the dearest);
  old-16        the effect of 16 fields the way it had to be done before: get_poses, membership and sums on the host (numpy),
                add_accelerations for every body reached, then the step.

Every field has strength zero, so every world computes the same trajectory as the one without fields and the differences are the
pass alone.  All worlds are warmed, then stepped in turns — `rounds` rounds of `chunk` steps each, the variants alternating — and a
step is timed by the host clock around phx_world_update + phx_world_synchronize.  Per variant: the median step, the 10th and 90th
percentile, and the spread of its per-round medians (max - min), which is the run-to-run noise a difference has to exceed.  Two
conditions are checked and reported: `none` equals `parent` within the parent's own spread, and field_passes() rose by exactly one
per step whatever the list's length.  The field kernel's own time comes from a kernel trace in a run of its own:
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/field_cost.py --only uniform-1,radial-1,uniform-16,radial-16,uniform-256,radial-256`.

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
from phyx_amd import Configuration, scenes, uniform_field, radial_field      # noqa: E402
from phyx_amd._lib import Config                                   # noqa: E402

DT = 1.0 / 60.0
G = -200.0
COUNTS = (1, 16, 256)


class Raw:
    """The few calls the loop needs, on any build of the library (the parent's knows no fields)."""

    def __init__(self, lib, scene):
        self.L = lib
        vp, f32, i32 = C.c_void_p, C.c_float, C.c_int32
        for name, res, args in (("phx_world_create", C.c_int, [C.POINTER(vp), C.c_int]), ("phx_world_destroy", None, [vp]),
                                ("phx_world_add_body", C.c_int, [vp, f32, f32, f32, f32, f32]), ("phx_world_set_body_static", C.c_int, [vp, i32]),
                                ("phx_world_set_gravity", C.c_int, [vp, f32]), ("phx_world_update", C.c_int, [vp, f32, C.POINTER(Config)]),
                                ("phx_world_synchronize", C.c_int, [vp]), ("phx_last_error", C.c_char_p, [])):
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

    def step(self, cfg):
        self.ok(self.L.phx_world_update(self.h, DT, C.byref(cfg)))
        self.ok(self.L.phx_world_synchronize(self.h))


def field_list(kind, count, extent):
    if kind == "uniform":
        return [uniform_field(0.0, 0.0, 0.0)] * count
    return [radial_field(0.0, -1000.0, 0.0, 8.0 * extent, disc=(0.0, 0.0, 4.0 * extent))] * count


def old_way(w, fields, n):
    """get_poses, membership and sums on the host, add_accelerations: what one step's fields took before the device pass."""
    p = w.poses()
    a = np.zeros((n, 3), dtype=np.float32)
    reached = np.zeros(n, dtype=bool)
    for f in fields:
        dx, dy = p[:, 0] - f["region"][0], p[:, 1] - f["region"][1]
        inside = dx * dx + dy * dy <= f["region"][2] * f["region"][2]
        rx, ry = p[:, 0] - f["value"][0], p[:, 1] - f["value"][1]
        d = np.sqrt(rx * rx + ry * ry)
        t = np.float32(1.0) - d / f["value"][3]
        on = inside & (d > np.float32(2.0 ** -10)) & (t > 0)
        mag = f["value"][2] * t
        with np.errstate(all="ignore"):
            a[:, 0] += np.where(on, rx / d * mag, 0)
            a[:, 1] += np.where(on, ry / d * mag, 0)
        reached |= on
    idx = np.flatnonzero(reached)[1:]                              # (body 0 is the ground: static, which the device skips by its inverse mass)
    w.add_accelerations(idx, a[idx])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libphyx_amd.so built at the parent commit")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--columns", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--only", help="comma-separated variants (default: all)")
    args = ap.parse_args()
    scene = scenes.stack(args.columns, args.rows)
    n = len(scene["px"])
    extent = 15.0 * args.columns + 10.0 * args.rows
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)._c()      # bench.py's cfg 2

    names = ["none"] + ["%s-%d" % (k, c) for c in COUNTS for k in ("uniform", "radial")] + ["old-16"]
    if args.parent_lib:
        names.insert(0, "parent")
    if args.only:
        names = [v for v in names if v in args.only.split(",")]
    worlds, before = {}, {}
    for name in names:
        if name == "parent":
            worlds[name] = Raw(C.CDLL(os.path.abspath(args.parent_lib)), scene)
            continue
        w = phyx_amd.World(0, gravity=G)
        w.add_scene(scene)
        if "-" in name and name != "old-16":
            kind, count = name.split("-")
            w.set_fields(field_list(kind, int(count), extent))
        worlds[name] = w
    old_fields = field_list("radial", 16, extent)

    def step(name):
        w = worlds[name]
        if name == "parent":
            w.step(cfg)
            return
        if name == "old-16":
            old_way(w, old_fields, n)
        phyx_amd.api.check(w.L.phx_world_update(w.h, DT, C.byref(cfg)))
        phyx_amd.api.check(w.L.phx_world_synchronize(w.h))

    for name in names:
        for _ in range(args.warmup):
            step(name)
        if name != "parent":
            before[name] = worlds[name].field_passes()
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:                                         # the variants alternate: drift of the machine touches all alike
            chunk = []
            for _ in range(args.chunk):
                t0 = time.perf_counter()
                step(name)
                chunk.append(time.perf_counter() - t0)
            times[name].append(chunk)

    out = {"scene": "stack(%d, %d)" % (args.columns, args.rows), "bodies": n, "warmup": args.warmup, "rounds": args.rounds, "chunk": args.chunk, "ms": {}}
    for name in names:
        t = 1e3 * np.array(times[name])
        medians = np.median(t, axis=1)
        out["ms"][name] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4),
                           "round_spread": round(float(medians.max() - medians.min()), 4)}
    steps = args.rounds * args.chunk
    passes = {name: worlds[name].field_passes() - before[name] for name in names if name != "parent"}
    out["field_passes_per_step"] = {name: p / steps for name, p in passes.items()}
    out["one_pass_per_step"] = all(p == (steps if name not in ("none", "old-16") else 0) for name, p in passes.items())
    if "parent" in names and "none" in names:
        diff = out["ms"]["none"]["median"] - out["ms"]["parent"]["median"]
        out["none_minus_parent_ms"] = round(diff, 4)
        out["none_within_parent_spread"] = bool(abs(diff) <= out["ms"]["parent"]["round_spread"])
    if "none" in names and "uniform-1" in names:
        out["bytes_per_body_1_field"] = 32                         # mpos read + the acceleration slot written, 16 B each
    final = {name: worlds[name].bodies.tobytes() for name in names if name not in ("parent", "old-16")}
    out["same_trajectory"] = len(set(final.values())) <= 1         # (zero-strength fields: every world ends where `none` ends)
    print(json.dumps(out))
    ok = out["one_pass_per_step"] and out["same_trajectory"] and out.get("none_within_parent_spread", True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
