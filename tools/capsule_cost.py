"""What capsule bodies cost, on one small pile in one process:

  boxes / circles / capsules   this library: the same pen of `columns` x `rows` bodies dropped between two posts, each body's frame box
                               {hx, hy} taken as a box, as a circle of radius hy, or as a capsule {hx, hy}: UpdateManifolds' AllBoxes,
                               BodyShapes and BodyCapsules instantiations;
  parent_a / parent_b          the circle pile on a library built at the parent commit (--parent-lib PATH), twice: two worlds of the
                               same bytes, whose difference is the run-to-run spread a difference has to exceed.

All worlds are warmed, then stepped in turns — `rounds` rounds of `chunk` steps each, the variants alternating — and a step is timed by
the host clock around phx_world_update + phx_world_synchronize.  Per variant: the median step, the 10th and 90th percentile and the
spread of its per-round medians.  One condition is checked: the circle world of this library against the parent's, within the larger of
the parent's own spread and the distance between its two runs (a circle world launches the kernels it launched before: the capsule
routines are instantiations of their own).  The three piles are different worlds (boxes stack, circles and capsules roll), so their
steps compare what a pile of each costs, not one routine against another.

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
from phyx_amd import Configuration                                 # noqa: E402
from phyx_amd._lib import Config                                   # noqa: E402

DT = 1.0 / 60.0
G = -200.0
BOX, CIRCLE, CAPSULE = 0, 1, 2


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("hx", C.c_float), ("hy", C.c_float)]


class Raw:
    """The pile on any build of the library, through the C ABI alone (the parent's library knows boxes and circles)."""

    def __init__(self, lib, kind, columns, rows, hx, hy):
        self.L = lib
        vp, f32, i32 = C.c_void_p, C.c_float, C.c_int32
        for name, res, args in (("phx_world_create", C.c_int, [C.POINTER(vp), C.c_int]), ("phx_world_destroy", None, [vp]),
                                ("phx_world_add_body", C.c_int, [vp, f32, f32, f32, f32, f32]), ("phx_world_set_body_static", C.c_int, [vp, i32]),
                                ("phx_world_add_bodies", C.c_int, [vp, vp, i32, C.POINTER(i32)]), ("phx_world_set_shapes", C.c_int, [vp, vp, vp, i32]),
                                ("phx_world_set_inverse_masses", C.c_int, [vp, vp, vp, i32]), ("phx_world_set_gravity", C.c_int, [vp, f32]),
                                ("phx_world_update", C.c_int, [vp, f32, C.POINTER(Config)]), ("phx_world_synchronize", C.c_int, [vp]),
                                ("phx_world_counts", C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
                                ("phx_last_error", C.c_char_p, [])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.h = vp()
        self.ok(lib.phx_world_create(C.byref(self.h), 0))
        self.ok(lib.phx_world_set_gravity(self.h, G))
        width = columns * (2.0 * hx + 1.0)
        for px, py, sx, sy in ((0.0, 0.0, width, 5.0), (-0.5 * width - 4.0, 200.0, 3.0, 200.0), (0.5 * width + 4.0, 200.0, 3.0, 200.0)):
            i = lib.phx_world_add_body(self.h, px, py, 0.0, sx, sy)
            self.ok(i)
            self.ok(lib.phx_world_set_body_static(self.h, i))
        ex = hy if kind == CIRCLE else hx
        spawn = np.array([[(c + 0.5 - 0.5 * columns) * (2.0 * hx + 1.0), 5.0 + hy + r * (2.0 * hy + 0.5) + 0.5, 0.05 * ((c + r) % 5 - 2), ex, hy]
                          for r in range(rows) for c in range(columns)], dtype=np.float32)
        first = C.c_int32(0)
        self.ok(lib.phx_world_add_bodies(self.h, spawn.ctypes.data, len(spawn), C.byref(first)))
        if kind != BOX:
            idx = np.arange(first.value, first.value + len(spawn), dtype=np.int32)
            shapes = (Shape * len(spawn))(*[Shape(kind, ex, hy)] * len(spawn))
            self.ok(lib.phx_world_set_shapes(self.h, idx.ctypes.data, C.addressof(shapes), len(spawn)))
            masses = phyx_amd.circle_inverse_masses(hy) if kind == CIRCLE else phyx_amd.capsule_inverse_masses(hx, hy)
            masses = np.ascontiguousarray(np.repeat(masses, len(spawn), axis=0))
            self.ok(lib.phx_world_set_inverse_masses(self.h, idx.ctypes.data, masses.ctypes.data, len(spawn)))

    def ok(self, st):
        if st < 0:
            raise RuntimeError("status %d: %s" % (st, self.L.phx_last_error().decode()))

    def manifolds(self):
        n = [C.c_int32(0) for _ in range(4)]
        self.ok(self.L.phx_world_counts(self.h, *[C.byref(x) for x in n]))
        return n[1].value


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
    worlds = {"boxes": Raw(here, BOX, args.columns, args.rows, 6.0, 3.0), "circles": Raw(here, CIRCLE, args.columns, args.rows, 6.0, 3.0),
              "capsules": Raw(here, CAPSULE, args.columns, args.rows, 6.0, 3.0)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        worlds["parent_a"] = Raw(parent, CIRCLE, args.columns, args.rows, 6.0, 3.0)
        worlds["parent_b"] = Raw(parent, CIRCLE, args.columns, args.rows, 6.0, 3.0)
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
            times[name].append(chunk)
    out = {"pile": "%d x %d bodies {6, 3}" % (args.columns, args.rows), "warmup": args.warmup, "rounds": args.rounds, "chunk": args.chunk, "ms": {},
           "manifolds": {name: worlds[name].manifolds() for name in names}}
    for name in names:
        t = 1e3 * np.array(times[name])
        medians = np.median(t, axis=1)
        out["ms"][name] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4),
                           "round_spread": round(float(medians.max() - medians.min()), 4)}
    if args.parent_lib:
        a, b, c = (out["ms"][k]["median"] for k in ("parent_a", "parent_b", "circles"))
        spread = max(abs(a - b), out["ms"]["parent_a"]["round_spread"], out["ms"]["parent_b"]["round_spread"])
        out["circles_minus_parent_ms"] = round(c - 0.5 * (a + b), 4)
        out["parent_spread_ms"] = round(spread, 4)
        out["circles_within_parent_spread"] = bool(abs(c - 0.5 * (a + b)) <= spread)
    print(json.dumps(out))
    return 0 if out.get("circles_within_parent_spread", True) else 1


if __name__ == "__main__":
    sys.exit(main())
