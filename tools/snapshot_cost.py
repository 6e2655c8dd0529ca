"""Cost of the device snapshots on the cfg 2 world (stack(1000, 200), 200 001 bodies) after 30 steps, once as it is ("plain") and once
with all three optional columns active ("columns"), against the checkpoint the library had before them:

  save        phx_world_save into a filled snapshot (its memory is reused);
  load        phx_world_load of that snapshot;
  old         the old checkpoint on the same world: the four getters, set_state, and (columns) the three getters and setters;
  update      one phx_world_update in the steady state (the cached schedule is reused);
  first_load  the first update after a load      } both rebuild the solver's schedule
  first_old   the first update after set_state   }

Every sample is taken two ways at once: `*_device_ms` between two HIP events recorded on the world's stream around the queued work, and
`*_host_ms` by the host clock around the call plus a synchronise.  (`old` has no device figure: it waits for the device several times
inside.)  Each figure is the median of --reps repetitions after --warm unrecorded ones; `update_spread_ms` is the distance between the
fastest and the slowest recorded update.  `bytes` are the sizes that move: what a save or load reads and writes in HBM, what the old path
sends over PCIe.  Samples of the different kinds alternate, so drift hits them alike.

  python tools/snapshot_cost.py [--reps 20] [--warm 3] [--steps 30] [--out profiles/snapshot_cost.json]      prints one JSON line
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median(xs):
    xs = sorted(xs)
    return round(xs[len(xs) // 2], 4)


class _Clock:
    """HIP events on the world's stream and the host clock, around the same work.  The events come from the HIP runtime the library
    itself is linked against (the one libamdhip64 of the process), through ctypes."""

    def __init__(self, world):
        import ctypes as C
        self.C = C
        self.world = world
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(world.stream_ptr())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            self._ok(self.hip.hipEventCreate(C.byref(e)))

    @staticmethod
    def _ok(status):
        if status != 0:
            raise RuntimeError("HIP runtime call failed with status %d" % status)

    def time(self, work, events=True):
        self.world.sync()
        t = time.perf_counter()
        if events:
            self._ok(self.hip.hipEventRecord(self.e0, self.stream))
        work()
        if events:
            self._ok(self.hip.hipEventRecord(self.e1, self.stream))
        self.world.sync()
        host = 1e3 * (time.perf_counter() - t)
        ms = self.C.c_float(0.0)
        if events:
            self._ok(self.hip.hipEventSynchronize(self.e1))
            self._ok(self.hip.hipEventElapsedTime(self.C.byref(ms), self.e0, self.e1))
        return host, (float(ms.value) if events else None)


def _measure(columns, a):
    import numpy as np
    import phyx_amd
    from phyx_amd import Configuration, Snapshot, scenes
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)      # bench.py's cfg 2
    dt = 1.0 / 60.0
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scenes.stack(1000, 200))
    n = w.counts()[0]
    if columns:
        idx = np.arange(1, n, 97)
        w.set_collision_filters(idx, category=2, mask=0xFFFFFFFF, group=0)
        w.set_materials(idx, friction=0.4, restitution=0.0)
        w.set_body_flags([n - 1], 0)
    for _ in range(a.steps):
        w.Update(dt, cfg)
    w.sync()
    clock = _Clock(w)
    snap = Snapshot(0)
    w.save(snap)

    def old():
        state = w.state()
        cols = (w.collision_filters(), w.materials(), w.body_flags()) if columns else None
        w.set_state(*state)
        if columns:
            every = np.arange(n)
            w.set_collision_filters(every, cols[0]["category"], cols[0]["mask"], cols[0]["group"])
            w.set_materials(every, cols[1]["friction"], cols[1]["restitution"])
            w.set_body_flags(every, cols[2])

    kinds = ("save", "load", "old", "update", "first_load", "first_old")
    host = {k: [] for k in kinds}
    dev = {k: [] for k in kinds}
    step = lambda: w.Update(dt, cfg)
    for rep in range(a.warm + a.reps):
        sample = {}
        step()                                          # (the world moves on between repetitions, as it does in an application)
        sample["update"] = clock.time(step)
        sample["save"] = clock.time(lambda: w.save(snap))
        step()
        sample["load"] = clock.time(lambda: w.load(snap))
        sample["first_load"] = clock.time(step)
        sample["old"] = clock.time(old, events=False)
        sample["first_old"] = clock.time(step)
        if rep >= a.warm:
            for k, (h, d) in sample.items():
                host[k].append(h)
                if d is not None:
                    dev[k].append(d)
    nb, nm, ncp, nj = snap.counts
    blob = len(snap.to_bytes())
    state_bytes = 128 * nb + 16 * nm + 32 * ncp + 20 * nj
    out = {"bodies": nb, "manifolds": nm, "joints": nj, "blob_bytes": blob,
           # (a save reads the arrays and, after a step, the 88 bytes of resident state per body, and writes the snapshot; a load reads the
           #  snapshot and writes the arrays, the resident state and 8 bytes per manifold for the pair set)
           "bytes": {"save_hbm_read_plus_written": 2 * (blob - 128) + 88 * nb,
                     "load_hbm_read_plus_written": 2 * (blob - 128) + 88 * nb + 8 * nm,
                     "old_pcie_down_plus_up": 2 * state_bytes + (2 * (12 + 8 + 4) * nb if columns else 0)},
           "update_spread_ms": round(max(host["update"]) - min(host["update"]), 4)}
    for k in kinds:
        out[k + "_host_ms"] = _median(host[k])
        if dev[k]:
            out[k + "_device_ms"] = _median(dev[k])
    out["save_plus_load_host_ms"] = round(out["save_host_ms"] + out["load_host_ms"], 4)
    out["old_over_save_plus_load"] = round(out["old_host_ms"] / out["save_plus_load_host_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_cost.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"reps": a.reps, "plain": _measure(False, a), "columns": _measure(True, a)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
