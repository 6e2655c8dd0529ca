"""Wall time of the World's queries on the cfg 2 world (stack(1000, 200), 200 001 bodies) after 30 warm-up steps, and the batch size
at which the index path overtakes the scan path, per kind of query:

  points   query_points (skip static), uniform over the stack;
  rays     raycast, uniform origins and directions, max_t 500;
  boxes    query_aabb, 60 x 60 boxes;
  shapes   query_boxes, 60 x 60 boxes at uniform angles;
  casts    cast_boxes, 10 x 10 boxes at uniform angles, uniform origins and directions, max_t 500;
  build    the query index alone (after a step moved every body: phx_world_query_index);
  brute    what an application has without the queries: get_bodies (25.6 MB over PCIe) and a numpy brute force of one pick.

Every kind runs at each batch size of COUNTS on both paths (PHX_QUERY_PATH=scan / index, one fresh world each).  A sample is the call
(host form: it waits for its results) after one Update and a stream synchronisation, so the index path pays its build every time (the
geometry moved): the cost an application that queries once per step sees.  `crossover_<kind>` is the smallest batch size of COUNTS from
which on the index path is faster at every larger size too (null: never).  `python tools/query_cost.py [--samples K] [--kinds a,b]
[--counts m,n]` prints one JSON line of median milliseconds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 64, 128, 256, 512, 1024, 2048, 4096, 10000)
KINDS = ("points", "rays", "boxes", "shapes", "casts")


def _world(path, warmup):
    import phyx_amd
    from phyx_amd import Configuration, scenes
    os.environ["PHX_QUERY_PATH"] = path
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)      # bench.py's cfg 2
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scenes.stack(1000, 200))
    for _ in range(warmup):
        w.Update(1.0 / 60.0, cfg)
    w.sync()
    return w, cfg


def _median(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 4)


def _queries(rng, kind, k):
    import numpy as np
    o = rng.uniform([-3000, 0], [3000, 2000], (k, 2))
    if kind == "points":
        return o.astype(np.float32)
    if kind == "boxes":
        return np.concatenate([o, o + 60.0], axis=1).astype(np.float32)
    t = rng.uniform(0, 6.283, k)
    ray = [np.stack([np.cos(t), np.sin(t)], axis=1), np.full((k, 1), 500.0)]
    if kind == "rays":
        return np.concatenate([o] + ray, axis=1).astype(np.float32)
    a = rng.uniform(0, 6.283, k)
    box = [o, np.stack([np.cos(a), np.sin(a), -np.sin(a), np.cos(a)], axis=1), np.full((k, 2), 30.0 if kind == "shapes" else 5.0)]
    return np.concatenate(box + (ray if kind == "casts" else []), axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    a = ap.parse_args()
    kinds, counts = a.kinds.split(","), [int(c) for c in a.counts.split(",")]
    sys.path.insert(0, ROOT)
    import numpy as np
    rng = np.random.default_rng(1)
    out = {"bodies": None, "counts": counts}
    call = {"points": lambda w, q: w.query_points(q, skip_static=True), "rays": lambda w, q: w.raycast(q), "boxes": lambda w, q: w.query_aabb(q),
            "shapes": lambda w, q: w.query_boxes(q), "casts": lambda w, q: w.cast_boxes(q)}
    for path in ("scan", "index"):
        w, cfg = _world(path, a.warmup)
        out["bodies"] = w.counts()[0]
        for kind in kinds:
            row = []
            for k in counts:
                ts = []
                for _ in range(a.samples):
                    q = _queries(rng, kind, k)
                    w.Update(1.0 / 60.0, cfg)
                    w.sync()
                    t = time.perf_counter()
                    call[kind](w, q)
                    ts.append(1e3 * (time.perf_counter() - t))
                row.append(_median(ts))
            out["%s_%s_ms" % (kind, path)] = row
        if path == "index":
            ts = []
            for _ in range(a.samples):
                w.Update(1.0 / 60.0, cfg)
                w.sync()
                t = time.perf_counter()
                w.query_index()
                w.sync()
                ts.append(1e3 * (time.perf_counter() - t))
            out["build_ms"] = _median(ts)
            ts = []
            for _ in range(a.samples):
                w.Update(1.0 / 60.0, cfg)
                w.sync()
                t = time.perf_counter()
                b = w.bodies
                p = np.float32(rng.uniform(-3000, 3000)), np.float32(rng.uniform(20, 1900))
                inside = ((b["aabb_min"]["x"] <= p[0]) & (b["aabb_max"]["x"] >= p[0]) & (b["aabb_min"]["y"] <= p[1]) & (b["aabb_max"]["y"] >= p[1]))
                np.flatnonzero(inside)
                ts.append(1e3 * (time.perf_counter() - t))
            out["brute_pick_ms"] = _median(ts)
        del w
    for kind in kinds:
        s, i = out["%s_scan_ms" % kind], out["%s_index_ms" % kind]
        cross = None
        for j in range(len(counts)):
            if all(i[m] < s[m] for m in range(j, len(counts))):
                cross = counts[j]
                break
        out["crossover_%s" % kind] = cross
    print(json.dumps(out))


if __name__ == "__main__":
    main()
