"""Child process of tests/test_units_gpu.py::test_set_comm_refuses_a_world_with_units: a one-rank native communicator and the units of
the kind named on the command line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phyx_amd                                   # noqa: E402
from phyx_amd import Configuration, PhxError, api, scenes      # noqa: E402
from unit_spec import KINDS                       # noqa: E402

ERR_STATE = -5
O = (0.0, 0.0)
# two units on scenes.stack(2, 4): one between boxes 1 and 2, one between box 3 and the world
RECORDS = {"pin": [(1, 2, (0.0, 5.0), (0.0, -5.0), O), (3, -1, O, (0.0, 45.0), O)],
           "link": [(1, 2, (0.0, 5.0), (0.0, -5.0), 1.0, 1.0, 0.0, 0.0, 0.0, 0), (3, -1, O, (0.0, 45.0), 0.0, 20.0, 0.0, 0.0, 0.0, 0)],
           "angle": [(1, 2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (3, -1, -0.5, 0.5, 0.0, 0.0, 1.0, 0.01, 0.0, 0.0)],
           "slider": [(1, 2, O, O, (1.0, 0.0), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0),
                      (3, -1, O, O, (0.0, 1.0), -50.0, 50.0, 0.0, 0.0, 1.0, 0.01, 0.0, 0.0, 0.0, 0)]}


def main(name):
    kind = next(k for k in KINDS if k.name == name)
    try:
        comm = api.Comm(api.Comm.unique_id(), 0, 1, 0)
    except PhxError as e:
        print("NO COMMUNICATOR:", e)
        return 0
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
    units = np.array(RECORDS[name], dtype=kind.dtype)
    for staged in ("host", "device"):
        pw = phyx_amd.World(0, gravity=-200.0)
        add, get, remove, count = (getattr(pw, m) for m in (kind.add, kind.get, kind.remove, kind.count))
        pw.add_scene(scenes.stack(2, 4))
        add(units)
        if staged == "device":
            pw.Update(1.0 / 60.0, cfg)
        before = (pw.bodies.tobytes(), get().tobytes(), pw.pin_schedule_builds())
        try:
            pw.set_comm(comm)
        except PhxError as e:
            assert e.status == ERR_STATE and kind.plural in str(e), e
        else:
            raise AssertionError("set_comm attached a world that holds " + kind.plural)
        assert (pw.bodies.tobytes(), get().tobytes(), pw.pin_schedule_builds()) == before, "the refusal changed the world (%s)" % staged
        pw.Update(1.0 / 60.0, cfg)                # still an unsharded world: the plain step runs
        assert count() == 2
        # without its units the world attaches, and then takes none
        remove([0, 1])
        pw.set_comm(comm)
        try:
            add(units)
        except PhxError as e:
            assert e.status == ERR_STATE, e
        else:
            raise AssertionError(kind.add + " on a communicator-attached world")
        assert count() == 0
        pw.set_comm(None)
        del pw, add, get, remove, count
    print(kind.plural + " comm worker ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
