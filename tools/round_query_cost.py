"""Wall time of the round queries beside the box queries they stand next to, in the manner of tools/query_cost.py, on two worlds of
200 001 bodies after 30 warm-up steps:

  cfg2     bench.py's cfg 2 world, stack(1000, 200): boxes only, no shape column;
  mixed    the same stack with every other body that can move a circle of radius 5 (set_shapes; the masses stay).

per kind of query:

  shapes       query_boxes, 60 x 60 boxes at uniform angles;
  circles      query_circles, radius 30 (the same reach across);
  casts        cast_boxes, 10 x 10 boxes at uniform angles, uniform origins and directions, max_t 500;
  disc_casts   cast_circles, radius 5, the same origins' and directions' distribution.

Every kind runs at each batch size of COUNTS on both paths (PHX_QUERY_PATH=scan / index, one fresh world each), the kinds in the order
given and each with its own seeded queries, so that a copy of this tool beside another build of the library (it imports the package
of the tree it lies in), run with --kinds shapes,casts, samples the same worlds with the same queries in the same order.
A sample is the call (host form: it waits for its results) after one Update and a stream synchronisation, so the index path pays its
build every time.  Per (world, kind, path) the output has the medians over --samples rounds in milliseconds and, as `spread`, the
largest (max - min) / median over the batch sizes; `crossover_<world>_<kind>` as in tools/query_cost.py.
`python tools/round_query_cost.py [--samples K] [--kinds a,b] [--counts m,n] [--worlds cfg2,mixed]` prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 64, 128, 256, 512, 1024, 2048, 4096, 10000)
KINDS = ("shapes", "circles", "casts", "disc_casts")
WORLDS = ("cfg2", "mixed")


def _world(name, path, warmup):
    import numpy as np
    import phyx_amd
    from phyx_amd import Configuration, scenes
    os.environ["PHX_QUERY_PATH"] = path
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)      # bench.py's cfg 2
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scenes.stack(1000, 200))
    if name == "mixed":
        w.set_shapes(np.arange(1, w.counts()[0], 2, dtype=np.int32), phyx_amd.SHAPE_CIRCLE, 5.0)
    for _ in range(warmup):
        w.Update(1.0 / 60.0, cfg)
    w.sync()
    return w, cfg


def _queries(rng, kind, k):
    import numpy as np
    o = rng.uniform([-3000, 0], [3000, 2000], (k, 2))
    t = rng.uniform(0, 6.283, k)
    ray = [np.stack([np.cos(t), np.sin(t)], axis=1), np.full((k, 1), 500.0)]
    if kind in ("circles", "disc_casts"):
        return np.concatenate([o, np.full((k, 1), 30.0 if kind == "circles" else 5.0)] + (ray if kind == "disc_casts" else []), axis=1).astype(np.float32)
    a = rng.uniform(0, 6.283, k)
    box = [o, np.stack([np.cos(a), np.sin(a), -np.sin(a), np.cos(a)], axis=1), np.full((k, 2), 30.0 if kind == "shapes" else 5.0)]
    return np.concatenate(box + (ray if kind == "casts" else []), axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    ap.add_argument("--worlds", default=",".join(WORLDS))
    a = ap.parse_args()
    kinds, counts, worlds = a.kinds.split(","), [int(c) for c in a.counts.split(",")], a.worlds.split(",")
    sys.path.insert(0, ROOT)
    import numpy as np
    call = {"shapes": lambda w, q: w.query_boxes(q), "casts": lambda w, q: w.cast_boxes(q),
            "circles": lambda w, q: w.query_circles(q), "disc_casts": lambda w, q: w.cast_circles(q)}
    out = {"bodies": None, "counts": counts, "samples": a.samples}
    for name in worlds:
        for path in ("scan", "index"):
            w, cfg = _world(name, path, a.warmup)
            out["bodies"] = w.counts()[0]
            for kind in kinds:
                row, spread, rng = [], 0.0, np.random.default_rng(1 + KINDS.index(kind))
                for k in counts:
                    ts = []
                    for _ in range(a.samples):
                        q = _queries(rng, kind, k)
                        w.Update(1.0 / 60.0, cfg)
                        w.sync()
                        t = time.perf_counter()
                        call[kind](w, q)
                        ts.append(1e3 * (time.perf_counter() - t))
                    ts.sort()
                    row.append(round(ts[len(ts) // 2], 4))
                    spread = max(spread, (ts[-1] - ts[0]) / ts[len(ts) // 2])
                out["%s_%s_%s_ms" % (name, kind, path)] = row
                out["%s_%s_%s_spread" % (name, kind, path)] = round(spread, 3)
            del w
        for kind in kinds:
            s, i = out["%s_%s_scan_ms" % (name, kind)], out["%s_%s_index_ms" % (name, kind)]
            out["crossover_%s_%s" % (name, kind)] = next((counts[j] for j in range(len(counts)) if all(i[m] < s[m] for m in range(j, len(counts)))), None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
