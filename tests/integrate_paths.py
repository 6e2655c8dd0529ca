"""IntegrateVelocity on each of the three kernels that carry it (csrc/body_view.h integrate_velocity): a world in lockstep with the oracle
World, `bodies` byte-equal after each of three steps.  test_integrate_velocity_gpu.py runs it in-process, and — as a child process, because
the library reads PHX_NO_SPLIT_SORT once — with the two-level sort off.

The scene is 601 bodies: two tiles of the dealing kernel (k_keys_buckets) and three buckets, so that the first update of a world cannot
take the two-level sort (no splitters on record yet: k_build_keys<true>) and the later ones do (k_keys_buckets<true, 2>).  Gravity, the
static ground and a few kinematic bodies (inverse masses zeroed) reach both sides of the `inv_mass > 0` test; with `accel`, accelerations
on a subset — static and kinematic bodies among them — before steps 1 and 3 feed the acceleration array to the kernel of that step."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phyx_amd                              # noqa: E402
from phyx_amd import Configuration, scenes   # noqa: E402
import spawn_lockstep                        # noqa: E402
from helpers import oracle_world             # noqa: E402

DT = 1.0 / 60.0
KINEMATIC = (7, 300, 600)
ACCELERATED = np.array([0, 1, 7, 255, 256, 300, 511, 512, 600], dtype=np.int32)      # the ground, kinematic bodies, both sides of a tile's edge


def _accelerations(step):
    k = np.arange(len(ACCELERATED), dtype=np.float32)
    return np.stack([100.0 + 7.0 * k + step, -50.0 + 11.0 * k, 0.5 * k - 1.0], axis=1).astype(np.float32)


def lockstep(oracle, timing, accel):
    scene = scenes.falling(600, width=6000.0)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
    pw = phyx_amd.World(0, gravity=-200.0)
    pw.add_scene(scene)
    ow = oracle_world(scene)
    assert len(ow.bodies()) == 601
    for i in KINEMATIC:
        pw.set_inverse_mass(i, 0.0, 0.0)
        b = ow.bodies(); b["inv_mass"][i] = 0.0; b["inv_inertia"][i] = 0.0
    if timing:
        pw.set_phase_timing(True)            # the World integrates velocities with a kernel of its own (k_integrate_velocity)
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    for step in range(3):
        if accel and step in (0, 2):
            a = _accelerations(step)
            pw.add_accelerations(ACCELERATED, a)
            b = ow.bodies()
            b["acceleration"]["x"][ACCELERATED] += a[:, 0]; b["acceleration"]["y"][ACCELERATED] += a[:, 1]; b["angular_acceleration"][ACCELERATED] += a[:, 2]
        spawn_lockstep.step(oracle, pw, ow, cfg, DT)
        assert pw.bodies.tobytes() == ow.bodies().tobytes(), "bodies differ after step %d (timing=%s, accel=%s)" % (step + 1, timing, accel)
    vy = pw.bodies["velocity"]["y"]
    assert vy[2] != 0.0 and (accel or not vy[list(KINEMATIC)].any())      # (gravity where there is mass, and only there)


def main():
    from oracle import binding
    from phyx_amd import _lib
    binding.set_arith(_lib.load().phx_arith_mode())
    for accel in (False, True):
        lockstep(binding, False, accel)
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
