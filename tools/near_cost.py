"""Wall time of the nearest-body query beside the point query on the same points, in the manner of tools/round_query_cost.py, on
bench.py's cfg 2 world (stack(1000, 200): 200 001 bodies) after 30 warm-up steps.

Per max_dist of 2, 50 and FLT_MAX ("near2", "near50", "nearmax") query_nearest runs at each batch size of COUNTS on both paths
(PHX_QUERY_PATH=scan / index, one fresh world each); "points" is query_points on the same points, the yardstick: that call is older
than this tool.  The points are uniform over the stack and 100 units above it, so a third of them lie above everything: under FLT_MAX
those are the walks only the running bound keeps short.  A sample is the call (host form: it waits for its results) after one Update
and a stream synchronisation, so the index path pays its build every time.  Per (kind, path) the output has the medians over
--samples rounds in milliseconds and, as `spread`, the largest (max - min) / median over the batch sizes; `crossover_<kind>` is the
smallest batch size from which the index is faster at every larger one (DeviceQuery::SCAN_MAX is the largest measured size below it).
`python tools/near_cost.py [--samples K] [--kinds a,b] [--counts m,n]` prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 64, 256, 512, 1024, 2048, 4096, 16384, 65536)
KINDS = ("points", "near2", "near50", "nearmax")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    a = ap.parse_args()
    kinds, counts = a.kinds.split(","), [int(c) for c in a.counts.split(",")]
    sys.path.insert(0, ROOT)
    import numpy as np
    reach = {"near2": 2.0, "near50": 50.0, "nearmax": float(np.finfo(np.float32).max)}
    out = {"bodies": None, "counts": counts, "samples": a.samples}
    for path in ("scan", "index"):
        w, cfg = _world(path, a.warmup)
        out["bodies"] = w.counts()[0]
        for kind in kinds:
            row, spread, rng = [], 0.0, np.random.default_rng(7)         # (every kind sees the same points)
            for k in counts:
                ts = []
                for _ in range(a.samples):
                    p = rng.uniform([-7600, 0], [7600, 2200], (k, 2)).astype(np.float32)
                    q = p if kind == "points" else np.concatenate([p, np.full((k, 1), reach[kind], dtype=np.float32)], axis=1)
                    w.Update(1.0 / 60.0, cfg)
                    w.sync()
                    t = time.perf_counter()
                    w.query_points(q) if kind == "points" else w.query_nearest(q)
                    ts.append(1e3 * (time.perf_counter() - t))
                ts.sort()
                row.append(round(ts[len(ts) // 2], 4))
                spread = max(spread, (ts[-1] - ts[0]) / ts[len(ts) // 2])
            out["%s_%s_ms" % (kind, path)] = row
            out["%s_%s_spread" % (kind, path)] = round(spread, 3)
        del w
    for kind in kinds:
        s, i = out["%s_scan_ms" % kind], out["%s_index_ms" % kind]
        out["crossover_%s" % kind] = next((counts[j] for j in range(len(counts)) if all(i[m] < s[m] for m in range(j, len(counts)))), None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
