"""Child process of tests/test_angles_gpu.py::test_set_comm_refuses_a_world_with_angles: a one-rank native communicator and the angles."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phyx_amd                                   # noqa: E402
from phyx_amd import Configuration, PhxError, api, scenes      # noqa: E402

ERR_STATE = -5


def main():
    try:
        comm = api.Comm(api.Comm.unique_id(), 0, 1, 0)
    except PhxError as e:
        print("NO COMMUNICATOR:", e)
        return 0
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
    angles = np.zeros(2, dtype=api.angle_dtype)
    angles[0] = (1, 2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    angles[1] = (3, -1, -0.5, 0.5, 0.0, 0.0, 1.0, 0.01, 0.0, 0.0)
    for staged in ("host", "device"):
        pw = phyx_amd.World(0, gravity=-200.0)
        pw.add_scene(scenes.stack(2, 4))
        pw.add_angles(angles)
        if staged == "device":
            pw.Update(1.0 / 60.0, cfg)
        before = (pw.bodies.tobytes(), pw.angles().tobytes(), pw.pin_schedule_builds())
        try:
            pw.set_comm(comm)
        except PhxError as e:
            assert e.status == ERR_STATE and "angles" in str(e), e
        else:
            raise AssertionError("set_comm attached a world that holds angles")
        assert (pw.bodies.tobytes(), pw.angles().tobytes(), pw.pin_schedule_builds()) == before, "the refusal changed the world (%s)" % staged
        pw.Update(1.0 / 60.0, cfg)                # still an unsharded world: the plain step runs
        assert pw.angle_count() == 2
        # without its angles the world attaches, and then takes no angle
        pw.remove_angles([0, 1])
        pw.set_comm(comm)
        try:
            pw.add_angles(angles)
        except PhxError as e:
            assert e.status == ERR_STATE, e
        else:
            raise AssertionError("add_angles on a communicator-attached world")
        assert pw.angle_count() == 0
        pw.set_comm(None)
        del pw
    print("angles comm worker ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
