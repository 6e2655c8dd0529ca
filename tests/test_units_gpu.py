"""What every kind of unit of the pin pass has alike on the device (include/phyx_amd.h PINS ... SLIDERS), once per kind of
unit_spec.KINDS: sharded worlds and communicators refuse units, set_state leaves none, a world that lost its units is a world without,
a snapshot with units has no blob; and the schedule call over the four kinds in one world.  What a kind has of its own - its paths, its
edits, its removals, its refusals - is in tests/test_<kind>s_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError, scenes
import angle_spec
import link_spec
import slider_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, NAMES, ERR_CAPACITY, ERR_STATE, O, X, Y
from unit_scenes import mixed_world
from unit_spec import KINDS

pytestmark = pytest.mark.gpu

by_kind = pytest.mark.parametrize("kind", KINDS, ids=[kind.name for kind in KINDS])

# one unit between box 1 of scenes.stack(2, 3) and the world (the pin: between boxes 1 and 2), as add_<kind>s takes it
ONE = {"pin": ul.pins([(1, 2, (0.0, 5.0), (0.0, -5.0))]),
       "link": link_spec.make_links([(1, -1, O, (0.0, 90.0), 0.0, 80.0)]),
       "angle": angle_spec.make_angles([(1, -1, -0.5, 0.5)]),
       "slider": slider_spec.make_sliders([(1, -1, O, O, Y, -0.5, 0.5)])}
# the unit of the blob test, where that is another record than ONE's
BLOB = dict(ONE, angle=[(1, -1, -0.5, 0.5)], slider=[(1, -1, O, O, X, -0.5, 0.5)])
# two units on scenes.stack(3, 6), one between two boxes and one against the world
TWO = {"pin": ul.pins([(1, 2, (0.0, 5.0), (0.0, -5.0)), (3, -1, O, (0.0, 50.0))]),
       "link": link_spec.make_links([(1, 2, (0.0, 5.0), (0.0, -5.0), 1.0, 1.0), (3, -1, O, (0.0, 50.0), 0.0, 10.0)]),
       "angle": [(1, 2, 0.0, 0.0), (3, -1, -0.2, 0.2, 0.0, 0.0, 1.0, 5.0)],
       "slider": [(1, 2, O, O, X, 0.0, 0.0), (3, -1, O, O, Y, -0.2, 0.2, 0.0, 0.0, 1.0, 5.0)]}


def _stack_world(columns, rows):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(columns, rows))
    return pw


@by_kind
def test_sharded_worlds_carry_no_units(built_lib, kind):
    if kind.name == "pin":
        pw = mixed_world("pin", links=3)
    else:
        pw = _stack_world(2, 3)
        getattr(pw, kind.add)(ONE[kind.name])
    with pytest.raises(PhxError) as e:
        pw.set_shard(0, 2)
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_set_shard: the world holds %s, which a sharded world does not carry" % kind.plural)
    n = pw.counts()[0]
    with pytest.raises(PhxError) as e:
        pw.reslab(np.arange(n, dtype=np.int64), n, (-1e9, 1e9))
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_reslab: the world holds %s, which a sharded world does not carry" % kind.plural)
    pw.set_shard(0, 1)
    sharded = _stack_world(2, 3)
    sharded.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        getattr(sharded, kind.add)(ONE[kind.name])
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_%s: a sharded world carries no %s" % (kind.add, kind.plural))
    assert getattr(sharded, kind.count)() == 0


@by_kind
def test_set_comm_refuses_a_world_with_units(built_lib, kind):
    """phx_world_set_comm with a one-rank communicator on a world that holds units: PHX_ERR_STATE, nothing changed; without them it
    attaches, and add_<kind>s is then refused.  In a child process, as the other tests that create a communicator: RCCL's bootstrap
    must not be able to hang the suite's process (the library gives up after PHX_COMM_TIMEOUT_S)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "units_comm_worker.py")
    env = dict(os.environ, PHX_COMM_TIMEOUT_S="60")
    for attempt in range(2):
        p = subprocess.run([sys.executable, worker, kind.name], env=env, capture_output=True, text=True, timeout=300)
        if "NO COMMUNICATOR" not in p.stdout:
            break
    if "NO COMMUNICATOR" in p.stdout:
        pytest.skip("no RCCL communicator on this box: " + p.stdout[-300:])
    assert p.returncode == 0 and "%s comm worker ok" % kind.plural in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


@by_kind
def test_set_state_leaves_no_unit(built_lib, kind):
    pw = mixed_world(kind.name)
    pw.Update(DT, ul.cfg())
    pw.set_state(*pw.state())
    assert ul.counts(pw) == [0] * len(KINDS) and len(getattr(pw, kind.get)()) == 0
    pw.Update(DT, ul.cfg())


@by_kind
def test_a_world_that_lost_its_units_is_a_world_without(built_lib, kind):
    cfg = ul.cfg()
    pa, pb = _stack_world(3, 6), _stack_world(3, 6)
    getattr(pa, kind.add)(TWO[kind.name])
    getattr(pa, kind.remove)([0, 1])
    assert getattr(pa, kind.count)() == 0
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        for name, x, y in zip(NAMES, pa.state(), pb.state()):
            assert x.tobytes() == y.tobytes(), "%s differ at step %d" % (name, s)
    assert pa.pin_schedule_builds() == 0, "no units: no schedule, no pass"
    assert pa.save().to_bytes() == pb.save().to_bytes(), "a snapshot without %s is what it was" % kind.plural


@by_kind
def test_a_snapshot_with_units_has_no_blob(built_lib, kind):
    pw = _stack_world(2, 3)
    getattr(pw, kind.add)(BLOB[kind.name])
    snap = pw.save()
    refusal = "the snapshot holds 1 %s, which the blob (layout version 1) does not carry" % kind.plural
    with pytest.raises(PhxError) as e:
        snap.to_bytes()
    assert e.value.status == ERR_STATE and refusal in str(e.value)
    n = C.c_size_t(0)
    assert pw.L.phx_snapshot_blob_bytes(snap.h, C.byref(n)) == ERR_STATE
    assert ul.message(pw) == "phx_snapshot_blob_bytes: " + refusal
    getattr(pw, kind.remove)([0])
    assert len(pw.save().to_bytes()) > 0


def test_the_schedule_call_needs_room_for_all_kinds(built_lib):
    pw = mixed_world(KINDS[-1].name)
    assert all(ul.counts(pw)), "the mixed world lacks a kind"
    n = sum(ul.counts(pw))
    nc, ng, lg = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert pw.L.phx_world_get_pin_schedule(pw.h, None, 0, None, 0, C.byref(nc), None, 0, C.byref(ng), C.byref(lg)) == 0
    order = np.zeros(n, dtype=np.int32)
    coff, goff = np.zeros(nc.value + 1, dtype=np.int32), np.zeros(ng.value + 1, dtype=np.int32)
    args = (coff.ctypes.data_as(C.c_void_p), len(coff), C.byref(nc), goff.ctypes.data_as(C.c_void_p), len(goff), C.byref(ng), C.byref(lg))
    assert pw.L.phx_world_get_pin_schedule(pw.h, order.ctypes.data_as(C.c_void_p), n - 1, *args) == ERR_CAPACITY
    assert ul.message(pw) == "phx_world_get_pin_schedule: arrays too small"
    assert pw.L.phx_world_get_pin_schedule(pw.h, order.ctypes.data_as(C.c_void_p), n, *args) == 0
    assert sorted(order.tolist()) == list(range(n))
