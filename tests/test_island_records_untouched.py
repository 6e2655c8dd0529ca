"""What a solve may write (MI355X): of a joint record the two accumulated impulses and nothing else, of a static body nothing at all.
The island kernel's set-up asks for joint 0, contact point 0 and body 0 on behalf of lanes that have no unit or no body (every request
unconditional, island_kernel_body.h) and throws the answers away; its write-back must still touch only what the lanes own."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration
import path_edges as pe
from helpers import SMALL_SCENES, is_static, presolve_state

pytestmark = pytest.mark.gpu

CONFIGS = [(phyx_amd.SOLVE_SCALAR, 0, 15, 15), (phyx_amd.SOLVE_SCALAR, 1, 15, 15), (2, 2, 20, 20), (2, 2, 7, 0)]


@pytest.mark.parametrize("name", list(SMALL_SCENES))
@pytest.mark.parametrize("config", CONFIGS)
def test_a_solve_writes_only_impulses_and_dynamic_bodies(built_lib, name, config):
    make, warm = SMALL_SCENES[name]
    bodies, cps, joints = presolve_state(make(), warm)
    solver = phyx_amd.Solver(0)
    b, cp, j = bodies.copy(), cps.copy(), joints.copy()
    solver.SolveJoints(b, cp, j, Configuration(*config))
    _, lds_groups = solver.groups()
    if name.startswith("stack") and config[1] == 2:
        assert lds_groups > 0, "the stacks are solved by the island kernel: this test is about it"
    for field in ("contact_point_index", "body1", "body2"):
        assert j[field].tobytes() == joints[field].tobytes(), "the solve changed the joints' %s" % field
    assert cp.tobytes() == cps.tobytes(), "the solve changed the contact points"
    static = is_static(bodies).astype(bool)
    assert static.any()
    assert b[static].tobytes() == bodies[static].tobytes(), "the solve wrote to a static body's record"
    # ... and it did solve: some impulse moved
    assert j["normal_acc"].tobytes() != joints["normal_acc"].tobytes() or config[2] == 0


def test_a_resident_solve_writes_only_impulses(built_lib):
    """The same on device-resident arrays solved twice (the second solve runs on the cached, self-verified schedule)."""
    make, warm = SMALL_SCENES["stack10x100"]
    bodies, cps, joints = presolve_state(make(), warm)
    solver = phyx_amd.Solver(0)
    db, dc, dj = (phyx_amd.DeviceArray(a) for a in (bodies, cps, joints))
    cfg = Configuration(2, 2, 20, 20)
    for _ in range(2):
        solver.SolveJointsDevice(db, dc, dj, cfg)
    j = dj.to_host()
    for field in ("contact_point_index", "body1", "body2"):
        assert j[field].tobytes() == joints[field].tobytes(), "the solve changed the joints' %s" % field
    assert dc.to_host().tobytes() == cps.tobytes()
    b = db.to_host()
    static = is_static(bodies).astype(bool)
    assert b[static].tobytes() == bodies[static].tobytes(), "the solve wrote to a static body's record"


@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("name", ["units_256", "units_257", "units_512_joints_1024"])
def test_full_and_half_empty_groups_write_only_impulses(built_lib, name, bits):
    """Where the lanes that ask on nobody's behalf are fewest and most: a group at the small shape's capacity exactly (256 units, no idle
    lane), the same plus one unit (the 512-lane shape, half of its lanes idle) and the big shape at capacity (tests/path_edges.py)."""
    bodies, cps, joints = pe.lds_state(name)
    solver = phyx_amd.Solver(0)
    if bits == 16:
        solver.set_body_state_bits(16)
    b, cp, j = bodies.copy(), cps.copy(), joints.copy()
    solver.SolveJoints(b, cp, j, Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_MULTIPLE, 6, 3))
    groups, lds_groups = solver.groups()
    assert lds_groups > 0 and int(groups[lds_groups]) == len(joints), "every joint of these scenes is solved by the island kernel"
    for field in ("contact_point_index", "body1", "body2"):
        assert j[field].tobytes() == joints[field].tobytes(), "the solve changed the joints' %s" % field
    assert cp.tobytes() == cps.tobytes(), "the solve changed the contact points"
    static = is_static(bodies).astype(bool)
    assert b[static].tobytes() == bodies[static].tobytes(), "the solve wrote to a static body's record"
    assert j["normal_acc"].tobytes() != joints["normal_acc"].tobytes()
