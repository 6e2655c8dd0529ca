"""Wall time of the World's contact reports on the cfg 2 world (stack(1000, 200), 200 001 bodies) after 30 warm-up steps, and the batch
size at which the index path overtakes the scan path:

  contacts  World.contacts of K random bodies (host form: it waits for its records), at each K of COUNTS on both paths
            (PHX_CONTACT_PATH=scan / index, one fresh world each);
  build     the contact index alone (after a step changed the contact cache: phx_world_contact_index);
  events    one contact_events call per step (the per-step touch events);
  markers   contact_markers_device into a device buffer, then a stream synchronisation;
  brute     what an application has without the reports: the manifold, contact-point, joint and body getters (what the reference's
            demo loop reads) over PCIe.

A sample is the call after one Update and a stream synchronisation, so the index path pays its build every time: the cost an application
that asks once per step sees.  `crossover` is the smallest K of COUNTS from which on the index path is faster at every larger K too
(null: never).  `python tools/contact_cost.py [--samples K]` prints one JSON line of median milliseconds
(--counts 256,512,1024 measures other batch sizes).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 4, 16, 64, 256, 1024, 4096, 16384, 65536)


def _world(path, warmup):
    import phyx_amd
    from phyx_amd import Configuration, scenes
    os.environ["PHX_CONTACT_PATH"] = path
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


def _timed(w, cfg, samples, fn):
    ts = []
    for _ in range(samples):
        w.Update(1.0 / 60.0, cfg)
        w.sync()
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return _median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--counts", type=str, default=",".join(str(k) for k in COUNTS), help="comma-separated batch sizes")
    a = ap.parse_args()
    counts = tuple(int(k) for k in a.counts.split(","))
    sys.path.insert(0, ROOT)
    import numpy as np
    from phyx_amd import DeviceBuffer
    rng = np.random.default_rng(1)
    out = {"bodies": None, "counts": list(counts)}
    for path in ("scan", "index"):
        w, cfg = _world(path, a.warmup)
        n, nm = w.counts()[0], w.counts()[1]
        out["bodies"], out["manifolds"] = n, nm
        out["contacts_%s_ms" % path] = [_timed(w, cfg, a.samples, lambda: w.contacts(rng.integers(0, n, k))) for k in counts]
        if path == "index":
            out["build_ms"] = _timed(w, cfg, a.samples, lambda: (w.contact_index(), w.sync()))
            w.contact_events()
            out["events_ms"] = _timed(w, cfg, a.samples, w.contact_events)
            buf = DeviceBuffer(24 * 8 * nm)                         # (room for twice today's manifolds: the count moves between steps)
            out["markers_ms"] = _timed(w, cfg, a.samples, lambda: (w.contact_markers_device(buf.address(), 8 * nm), w.sync()))
            out["brute_getters_ms"] = _timed(w, cfg, a.samples, w.state)
        del w
    s, i = out["contacts_scan_ms"], out["contacts_index_ms"]
    cross = None
    for j in range(len(counts)):
        if all(i[m] < s[m] for m in range(j, len(counts))):
            cross = counts[j]
            break
    out["crossover"] = cross
    print(json.dumps(out))


if __name__ == "__main__":
    main()
