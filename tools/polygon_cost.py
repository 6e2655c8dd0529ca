"""What convex polygon bodies cost, on one small pile in one process:

  boxes / circles / capsules   this library: tools/capsule_cost.py's pen of `columns` x `rows` bodies dropped between two posts, each
                               body's frame box {hx, hy} taken as a box, as a circle of radius hy, or as a capsule {hx, hy}:
                               UpdateManifolds' AllBoxes, BodyShapes and BodyCapsules instantiations;
  polygons4 / hexagons         the same pen with every body a 4-gon of the box's corners (the same outline as `boxes`, through the
                               polygon routines) or a hexagon inscribed in the frame box: the BodyPolygons instantiation;
  parent_*_a / parent_*_b      the box, circle and capsule piles on a library built at the parent commit (--parent-lib PATH), each
                               twice: two worlds of the same bytes, whose difference is the run-to-run spread a difference has to exceed.

All worlds are warmed, then stepped in turns — `rounds` rounds of `chunk` steps each, the variants alternating — and a step is timed by
the host clock around phx_world_update + phx_world_synchronize.  Per variant: the median step, the 10th and 90th percentile and the
spread of its per-round medians.  One condition is checked per older kind: this library's pile against the parent's, within the larger
of the parent's own spread and the distance between its two runs (a world without polygons launches the kernels it launched before).
The polygon piles are reported against the box pile; no target is fixed.

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
from capsule_cost import BOX, CAPSULE, CIRCLE, DT, Raw             # noqa: E402

POLYGON = 3


class Polygons(Raw):
    """The pen as boxes, then every body made a polygon of the given body-local vertices."""

    def __init__(self, lib, vertices, columns, rows, hx, hy):
        Raw.__init__(self, lib, BOX, columns, rows, hx, hy)
        lib.phx_world_set_polygons.restype, lib.phx_world_set_polygons.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        n = columns * rows
        idx = np.arange(3, 3 + n, dtype=np.int32)                   # (behind the floor and the two posts)
        p = np.zeros(n, dtype=phyx_amd.polygon_dtype)
        p["count"] = len(vertices)
        p["v"][:, :len(vertices)] = np.asarray(vertices, dtype=np.float32)
        self.ok(lib.phx_world_set_polygons(self.h, idx.ctypes.data, p.ctypes.data, n))
        masses = np.ascontiguousarray(np.repeat(phyx_amd.polygon_inverse_masses(vertices).reshape(1, 2), n, axis=0))
        self.ok(lib.phx_world_set_inverse_masses(self.h, idx.ctypes.data, masses.ctypes.data, n))


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
    corners = [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)]
    hexagon = [(-0.5 * hx, -hy), (0.5 * hx, -hy), (hx, 0.0), (0.5 * hx, hy), (-0.5 * hx, hy), (-hx, 0.0)]
    older = {"boxes": BOX, "circles": CIRCLE, "capsules": CAPSULE}
    worlds = {name: Raw(here, kind, *size) for name, kind in older.items()}
    worlds["polygons4"] = Polygons(here, corners, *size)
    worlds["hexagons"] = Polygons(here, hexagon, *size)
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name, kind in older.items():
            for run in "ab":
                worlds["parent_%s_%s" % (name, run)] = Raw(parent, kind, *size)
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
    box = out["ms"]["boxes"]["median"]
    out["polygons4_over_boxes"] = round(out["ms"]["polygons4"]["median"] / box, 4)
    out["hexagons_over_boxes"] = round(out["ms"]["hexagons"]["median"] / box, 4)
    ok = True
    if args.parent_lib:
        for name in older:
            a, b, c = (out["ms"][k]["median"] for k in ("parent_%s_a" % name, "parent_%s_b" % name, name))
            spread = max(abs(a - b), out["ms"]["parent_%s_a" % name]["round_spread"], out["ms"]["parent_%s_b" % name]["round_spread"])
            within = bool(abs(c - 0.5 * (a + b)) <= spread)
            out[name + "_vs_parent"] = {"minus_parent_ms": round(c - 0.5 * (a + b), 4), "parent_spread_ms": round(spread, 4), "within": within}
            ok = ok and within
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
