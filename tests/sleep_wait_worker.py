"""Child process of tests/test_sleep_gpu.py::test_a_sleeping_world_waits_no_more_often_than_a_plain_one (PHX_WAIT_CLOCK=1 must be in the
environment before the library's first readback): the host waits of 50 steps of a fully asleep world, and of the same world with
sleeping off — its twin by the contract, every mobile body made static by set_inverse_masses / set_velocities.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phyx_amd                                   # noqa: E402
from phyx_amd import Configuration, _lib, scenes  # noqa: E402

DT = 1.0 / 60.0


def waits(L):
    ns, calls = C.c_longlong(0), C.c_longlong(0)
    L.phx_debug_wait_clock(C.byref(ns), C.byref(calls))
    return calls.value


def main():
    L = _lib.load()
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
    sc = scenes.stack(4, 6)
    mobile = np.flatnonzero(~sc["static"])
    on, off = phyx_amd.World(0, gravity=-200.0), phyx_amd.World(0, gravity=-200.0)
    for w in (on, off):
        w.add_scene(sc)
    on.set_sleeping(20.0, 5.0, 3 * DT)
    for _ in range(8):
        on.Update(DT, cfg)
        off.Update(DT, cfg)
    asleep = on.sleep_counts()[0]
    off.set_inverse_masses(mobile, np.zeros((len(mobile), 2), dtype=np.float32))
    off.set_velocities(mobile, np.zeros((len(mobile), 3), dtype=np.float32))
    counts = {}
    for name, w in (("waits_on", on), ("waits_off", off)):
        for _ in range(4):                       # (the rebuild after the change of the static set is behind both)
            w.Update(DT, cfg)
        w.sync()
        before = waits(L)
        for _ in range(50):
            w.Update(DT, cfg)
        w.sync()
        counts[name] = waits(L) - before
    print(json.dumps(dict(counts, asleep=int(asleep), mobile=int(len(mobile)), still_asleep=int(on.sleep_counts()[0]))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
