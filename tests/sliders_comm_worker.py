"""Child process of tests/test_sliders_gpu.py::test_set_comm_refuses_a_world_with_sliders: a one-rank native communicator and the sliders."""
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
    sliders = np.zeros(2, dtype=api.slider_dtype)
    sliders[0] = (1, 2, (0.0, 0.0), (0.0, 0.0), (1.0, 0.0), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0)
    sliders[1] = (3, -1, (0.0, 0.0), (0.0, 0.0), (0.0, 1.0), -50.0, 50.0, 0.0, 0.0, 1.0, 0.01, 0.0, 0.0, 0.0, 0)
    for staged in ("host", "device"):
        pw = phyx_amd.World(0, gravity=-200.0)
        pw.add_scene(scenes.stack(2, 4))
        pw.add_sliders(sliders)
        if staged == "device":
            pw.Update(1.0 / 60.0, cfg)
        before = (pw.bodies.tobytes(), pw.sliders().tobytes(), pw.pin_schedule_builds())
        try:
            pw.set_comm(comm)
        except PhxError as e:
            assert e.status == ERR_STATE and "sliders" in str(e), e
        else:
            raise AssertionError("set_comm attached a world that holds sliders")
        assert (pw.bodies.tobytes(), pw.sliders().tobytes(), pw.pin_schedule_builds()) == before, "the refusal changed the world (%s)" % staged
        pw.Update(1.0 / 60.0, cfg)                # still an unsharded world: the plain step runs
        assert pw.slider_count() == 2
        # without its sliders the world attaches, and then takes no slider
        pw.remove_sliders([0, 1])
        pw.set_comm(comm)
        try:
            pw.add_sliders(sliders)
        except PhxError as e:
            assert e.status == ERR_STATE, e
        else:
            raise AssertionError("add_sliders on a communicator-attached world")
        assert pw.slider_count() == 0
        pw.set_comm(None)
        del pw
    print("sliders comm worker ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
