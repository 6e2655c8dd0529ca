"""Pins on the device (include/phyx_amd.h PINS) held to their specification, tests/pin_spec.py: the device World and the oracle World in
lockstep, the spec applied to the oracle's bodies between its pre_solve and its solve on the device's own pin schedule, every byte of
the state and of the pins' impulses compared after every step; then the schedule's paths, the life cycle by twins, and the refusals."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, PhxError, scenes
from phyx_amd.api import pin_dtype
from helpers import oracle_world
from spawn_lockstep import compare
import pin_spec
import removal_spec

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
ITERS = 8
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
ERR_INVALID, ERR_STATE = -1, -5


def _cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def _scene(rows):
    """rows (px, py, half_x, half_y, static) -> a scenes.py dict"""
    r = np.asarray([(a, b, c, d) for a, b, c, d, _ in rows], dtype=np.float32).reshape(-1, 4)
    return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": np.zeros(len(rows), dtype=np.float32), "sx": r[:, 2].copy(), "sy": r[:, 3].copy(),
            "static": np.asarray([bool(s) for *_, s in rows], dtype=bool)}


def _join(base, rows):
    extra = _scene(rows)
    return {k: np.concatenate([base[k], extra[k]]) for k in ("px", "py", "angle", "sx", "sy", "static")}


def _pins(rows):
    p = np.zeros(len(rows), dtype=pin_dtype)
    for k, (a, b, a1, a2) in enumerate(rows):
        p[k] = (a, b, a1, a2, (0.0, 0.0))
    return p


def _chain(first_body, links, top, hang_from=-1, hang_anchor=None, spacing=10.0):
    """`links` boxes of 6 x 2 laid level with `top`, to its right, body numbers from first_body on; the first hangs from the world point
    `top` or from the point `hang_anchor` (its own frame) of body `hang_from`.  -> (body rows, pin rows).  The links are short of their
    joints (pins do not keep neighbours from colliding: only a sharp fold makes them touch)."""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(links)]
    pins = [(first_body, hang_from, (-h, 0.0), top if hang_from < 0 else hang_anchor)]
    pins += [(first_body + k, first_body + k - 1, (-h, 0.0), (h, 0.0)) for k in range(1, links)]
    return bodies, pins


def _worlds(scene, pins, gravity=G, with_oracle=True):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    got = pw.add_pins(pins)
    assert got.tolist() == list(range(len(pins)))
    return pw, (oracle_world(scene, gravity) if with_oracle else None)


def _step(oracle, pw, ow, cfg, pins, dt=DT):
    """spawn_lockstep.step with the pins: 1. pw.Update  2. ow.pre_solve  3. pin_spec on ow.bodies() on the device's own pin schedule
    4. the oracle's solver on the device's contact schedule  5. ow.integrate_position.  `pins` is the spec's own list."""
    sched = pw.pin_schedule()
    assert sorted(sched["order"].tolist()) == list(range(len(pins)))
    pw.Update(dt, cfg)
    ow.pre_solve(dt)
    pin_spec.solve(ow.bodies(), pins, sched["order"], dt, pw.pin_iterations)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(dt)
    return sched


def _lockstep(oracle, pw, ow, cfg, pins, steps, watch=slice(None)):
    """-> (the last schedule, the lowest pos.y the bodies `watch` reached)"""
    lowest = np.inf
    for s in range(steps):
        sched = _step(oracle, pw, ow, cfg, pins)
        compare(pw, ow, s)
        assert pw.pins().tobytes() == pins.tobytes(), "pins differ at step %d" % s
        lowest = min(lowest, float(ow.bodies()["pos"]["y"][watch].min()))
    return sched, lowest


def test_one_body_on_a_world_pin(oracle, built_lib):
    bodies, rows = _chain(0, 1, (0.0, 100.0))
    pins = _pins(rows)
    pw, ow = _worlds(_scene(bodies), pins)
    assert pw.pin_iterations == ITERS and pw.pin_count() == 1
    assert pw.pins().tobytes() == pins.tobytes(), "before the first step the pins wait on the host"
    sched, lowest = _lockstep(oracle, pw, ow, _cfg(), pins, 60)
    assert sched["lds_groups"] == 1 and len(sched["class_offsets"]) == 2
    assert np.abs(pins["impulse"]).max() > 0 and lowest < 96.0, "the pendulum never swung"


def test_chains_and_pairs(oracle, built_lib):
    """a pair of dynamic bodies, a 3-chain (two classes) and a 12-chain hung from a static body"""
    bodies = [(-100.0, 200.0, 4.0, 1.5, False), (-90.0, 200.0, 6.0, 2.0, False)]
    rows = [(0, 1, (5.0, 1.0), (-5.0, 0.0))]
    b3, p3 = _chain(2, 3, (0.0, 200.0))
    bodies += b3; rows += p3
    bodies += [(200.0, 200.0, 5.0, 5.0, True)]
    b12, p12 = _chain(6, 12, (205.0, 200.0), hang_from=5, hang_anchor=(5.0, 0.0))
    bodies += b12; rows += p12
    pins = _pins(rows)
    pw, ow = _worlds(_scene(bodies), pins)
    sched, lowest = _lockstep(oracle, pw, ow, _cfg(), pins, 40, watch=slice(6, None))
    assert sched["lds_groups"] == 1 and len(sched["group_offsets"]) == 2
    assert len(sched["class_offsets"]) - 1 == 2, "chains need two classes"
    b = pw.bodies
    assert (b["pos"]["x"][5], b["pos"]["y"][5]) == (200.0, 200.0), "the static body moved"
    assert lowest < 190.0, "the chain never swung"


@pytest.mark.parametrize("mode", list(MODES))
def test_pins_among_contacts(oracle, built_lib, mode):
    """scenes.stack(4, 10), an 8-chain dropped onto it, two neighbouring boxes of a column pinned to each other; the world pin's
    anchor moves at step 20"""
    base = scenes.stack(4, 10)
    n = len(base["px"])
    chain_bodies, rows = _chain(n, 8, (-45.0, 135.0))
    rows += [(4, 5, (0.0, 5.0), (0.0, -5.0))]
    pins = _pins(rows)
    pw, ow = _worlds(_join(base, chain_bodies), pins)

    def at(s):
        if s == 20:
            moved = np.array([[-5.0, 0.0, -40.0, 138.0]], dtype=np.float32)
            pw.set_pin_anchors([0], moved)
            pins["anchor1"][0], pins["anchor2"][0] = moved[0, :2], moved[0, 2:]

    builds = None
    for s in range(40):
        at(s)
        _step(oracle, pw, ow, _cfg(MODES[mode]), pins)
        compare(pw, ow, s)
        assert pw.pins().tobytes() == pins.tobytes(), "pins differ at step %d" % s
        builds = builds or pw.pin_schedule_builds()
    assert pw.pin_schedule_builds() == builds == 1, "an anchor edit keeps the schedule"
    m = pw.manifolds
    assert ((m["body1"] >= n) | (m["body2"] >= n)).any(), "the chain never touched the stack"


def _pairs(count):
    bodies, rows = [], []
    for k in range(count):
        x, y = 40.0 * (k % 20), 30.0 * (k // 20)
        bodies += [(x, y, 4.0, 1.5, False), (x + 10.0, y, 3.0 + (k % 3), 2.0, False)]
        rows += [(2 * k, 2 * k + 1, (5.0, 1.0 - 0.1 * (k % 7)), (-5.0, 0.0))]
    return bodies, rows


@pytest.mark.parametrize("case", ["pairs300_cap64", "chain40_cap16", "chain40", "pairs5_chain40_cap16"])
def test_the_paths(oracle, built_lib, monkeypatch, case):
    """several LDS groups; the trailing group out of HBM; one workgroup; an LDS group AND an active trailing group (whose slots then
    start behind the LDS group's: the absolute slot offsets and the work array's base)"""
    if case == "pairs300_cap64":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "64")
        bodies, rows = _pairs(300)
        steps, lds, groups = 6, 5, 5
    elif case == "pairs5_chain40_cap16":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
        bodies, rows = _pairs(5)
        chain_bodies, chain_rows = _chain(10, 40, (0.0, 500.0))
        bodies, rows = bodies + chain_bodies, rows + chain_rows
        steps, lds, groups = 12, 1, 2
    else:
        if case == "chain40_cap16":
            monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
        bodies, rows = _chain(0, 40, (0.0, 500.0))
        steps = 12
        lds, groups = (0, 1) if case == "chain40_cap16" else (1, 1)
    pins = _pins(rows)
    pw, ow = _worlds(_scene(bodies), pins)
    sched, _ = _lockstep(oracle, pw, ow, _cfg(), pins, steps)
    assert sched["lds_groups"] == lds and len(sched["group_offsets"]) - 1 == groups
    assert np.abs(pins["impulse"]).max() > 0
    if case == "pairs5_chain40_cap16":
        assert sched["group_offsets"].tolist() == [0, 5, 45], "the pairs in one LDS group, the chain behind them in the trailing group"
        assert np.abs(pins["impulse"][:5]).max() > 0 and np.abs(pins["impulse"][5:]).max() > 0, "both groups are active"


@pytest.mark.parametrize("value", ["0", "257", "x", ""])
def test_group_pins_knob_refuses_other_values(built_lib, monkeypatch, value):
    monkeypatch.setenv("PHX_PIN_GROUP_PINS", value)
    with pytest.raises(PhxError) as e:
        phyx_amd.World(0)
    assert e.value.status == ERR_INVALID


# ---- the life cycle, by twins ----
def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)
    assert a.pins().tobytes() == b.pins().tobytes(), "pins differ %s" % what


def _chain_world(links=12, extra_pair=True):
    bodies, rows = _chain(0, links, (0.0, 300.0))
    if extra_pair:
        bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-90.0, 300.0, 4.0, 1.5, False)]
        rows += [(links, links + 1, (5.0, 1.0), (-5.0, 0.0))]
    pw, _ = _worlds(_scene(bodies), _pins(rows), with_oracle=False)
    return pw


def test_remove_bodies_through_a_chain(built_lib):
    cfg = _cfg()
    pa = _chain_world()
    for _ in range(10):
        pa.Update(DT, cfg)
    state, pins = pa.state(), pa.pins()
    removed = [5]
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)
    keep = np.array([new[p["body1"]] >= 0 and (p["body2"] < 0 or new[p["body2"]] >= 0) for p in pins])
    kept = pins[keep].copy()
    kept["body1"] = new[kept["body1"]]
    kept["body2"] = np.where(kept["body2"] < 0, -1, new[np.maximum(kept["body2"], 0)])
    assert len(kept) == len(pins) - 2
    remap = pa.remove_bodies(removed)
    assert remap.tolist() == new.tolist()
    assert pa.pins().tobytes() == kept.tobytes()
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*filtered[0])
    pb.add_pins(kept)
    _same(pa, pb, "right after the removal")
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at step %d after the removal" % s)


def test_remove_pins(built_lib):
    cfg = _cfg()
    pa = _chain_world()
    for _ in range(5):
        pa.Update(DT, cfg)
    state, pins = pa.state(), pa.pins()
    builds = pa.pin_schedule_builds()
    pa.remove_pins([12, 3])
    kept = np.delete(pins, [3, 12])
    assert pa.pins().tobytes() == kept.tobytes(), "the others keep their order"
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*state)
    pb.add_pins(kept)
    for s in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at step %d after remove_pins" % s)
    assert pa.pin_schedule_builds() == builds + 1


def test_what_rebuilds_the_schedule(built_lib):
    cfg = _cfg()
    pw = _chain_world()
    pw.Update(DT, cfg)
    builds = pw.pin_schedule_builds()
    assert builds == 1
    pw.set_pin_anchors([0], np.array([[-5.0, 0.0, 2.0, 301.0]], dtype=np.float32))
    pw.add_bodies(np.array([[500.0, 500.0, 0.0, 2.0, 2.0]], dtype=np.float32))
    pw.set_velocities([1], np.array([[1.0, 0.0, 0.0]], dtype=np.float32))
    pw.Update(DT, cfg)
    assert pw.pin_schedule_builds() == builds, "anchor edits, spawns and the other edits keep the schedule"
    assert pw.pins()["anchor2"][0].tolist() == [2.0, 301.0]
    b = pw.bodies
    pw.set_inverse_masses([3], np.array([[b["inv_mass"][3], b["inv_inertia"][3]]], dtype=np.float32))
    pw.Update(DT, cfg)
    assert pw.pin_schedule_builds() == builds + 1, "set_inverse_masses rebuilds it"


def test_a_pin_whose_bodies_became_static(built_lib):
    cfg = _cfg()
    pw = _chain_world(links=3)
    for _ in range(5):
        pw.Update(DT, cfg)
    assert np.abs(pw.pins()["impulse"][3]).max() > 0
    pw.set_velocities([3, 4], np.zeros((2, 3), dtype=np.float32))
    pw.set_inverse_masses([3, 4], np.zeros((2, 2), dtype=np.float32))
    before = pw.bodies[[3, 4]]
    for _ in range(3):
        pw.Update(DT, cfg)
    after = pw.bodies[[3, 4]]
    assert after["pos"].tobytes() == before["pos"].tobytes() and after["velocity"].tobytes() == before["velocity"].tobytes(), "static bodies moved"
    pins = pw.pins()
    assert pins["impulse"][3].tolist() == [0.0, 0.0], "an inactive pin reads impulse 0"
    assert np.abs(pins["impulse"][:3]).max() > 0


def test_set_state_leaves_no_pin(built_lib):
    pw = _chain_world()
    pw.Update(DT, _cfg())
    pw.set_state(*pw.state())
    assert pw.pin_count() == 0 and len(pw.pins()) == 0
    pw.Update(DT, _cfg())


def test_save_load_and_fork(built_lib):
    cfg = _cfg()
    pw = _chain_world()
    pw.pin_iterations = 6
    for _ in range(5):
        pw.Update(DT, cfg)
    snap = pw.save()
    saved_pins = pw.pins()
    first = []
    for _ in range(10):
        pw.Update(DT, cfg)
        first.append((pw.bodies.tobytes(), pw.pins().tobytes()))
    other = phyx_amd.World(0, gravity=G)
    other.pin_iterations = 6
    other.load(snap)
    pw.load(snap)
    assert pw.pins().tobytes() == saved_pins.tobytes() == other.pins().tobytes()
    for s in range(10):
        pw.Update(DT, cfg)
        other.Update(DT, cfg)
        assert (pw.bodies.tobytes(), pw.pins().tobytes()) == first[s], "the loaded world differs at step %d" % s
        assert (other.bodies.tobytes(), other.pins().tobytes()) == first[s], "the fork differs at step %d" % s
    with pytest.raises(PhxError) as e:
        snap.to_bytes()
    assert e.value.status == ERR_STATE and "pins" in str(e.value)


def test_a_world_that_lost_its_pins_is_a_world_without(built_lib):
    cfg = _cfg()
    sc = scenes.stack(3, 6)
    pa, pb = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    pa.add_scene(sc); pb.add_scene(sc)
    pa.add_pins(_pins([(1, 2, (0.0, 5.0), (0.0, -5.0)), (3, -1, (0.0, 0.0), (0.0, 50.0))]))
    pa.remove_pins([0, 1])
    assert pa.pin_count() == 0
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        for name, x, y in zip(NAMES, pa.state(), pb.state()):
            assert x.tobytes() == y.tobytes(), "%s differ at step %d" % (name, s)
    assert pa.pin_schedule_builds() == 0
    assert pa.save().to_bytes() == pb.save().to_bytes(), "a snapshot without pins is what it was"


# ---- the refusals ----
def _unchanged(pw, before):
    bodies, pins, builds = before
    assert pw.bodies.tobytes() == bodies and pw.pins().tobytes() == pins and pw.pin_schedule_builds() == builds


def _raw_add(pw, pins, count=None, null=False):
    import ctypes as C
    p = np.ascontiguousarray(pins, dtype=pin_dtype)
    return pw.L.phx_world_add_pins(pw.h, None if null else p.ctypes.data_as(C.c_void_p), len(p) if count is None else count, None)


@pytest.mark.parametrize("staged", ["host", "device"])
def test_rejections_leave_the_world_unchanged(built_lib, staged):
    import ctypes as C
    cfg = _cfg()
    pw = _chain_world(links=4)
    if staged == "device":
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = (pw.bodies.tobytes(), pw.pins().tobytes(), pw.pin_schedule_builds())
    good = (0, 1, (1.0, 0.0), (0.0, 1.0), (0.0, 0.0))
    bad = [(-1, 1), (n, 1), (0, n), (0, -2), (2, 2)]
    for b1, b2 in bad:
        p = np.array([good, (b1, b2, (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))], dtype=pin_dtype)
        assert _raw_add(pw, p) == ERR_INVALID, (b1, b2)
        _unchanged(pw, before)
    for field, value in (("anchor1", np.nan), ("anchor2", np.inf), ("impulse", -np.inf)):
        p = np.array([good, good], dtype=pin_dtype)
        p[field][1][1] = value
        assert _raw_add(pw, p) == ERR_INVALID, field
        _unchanged(pw, before)
    assert _raw_add(pw, np.array([good], dtype=pin_dtype), count=-1) == ERR_INVALID
    assert _raw_add(pw, np.array([good], dtype=pin_dtype), null=True) == ERR_INVALID
    assert _raw_add(pw, np.zeros(0, dtype=pin_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    _unchanged(pw, before)
    np_ = pw.pin_count()
    for which in ([np_], [-1], [1, 1]):
        with pytest.raises(PhxError) as e:
            pw.remove_pins(which)
        assert e.value.status == ERR_INVALID
        with pytest.raises(PhxError) as e:
            pw.set_pin_anchors(which, np.zeros((len(which), 4), dtype=np.float32))
        assert e.value.status == ERR_INVALID
        _unchanged(pw, before)
    with pytest.raises(PhxError) as e:
        pw.set_pin_anchors([0], np.array([[0.0, np.nan, 0.0, 0.0]], dtype=np.float32))
    assert e.value.status == ERR_INVALID
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_pins(pw.h, None, 1) == ERR_INVALID
    assert pw.L.phx_world_remove_pins(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID
    assert pw.L.phx_world_set_pin_anchors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    pw.remove_pins([]); pw.set_pin_anchors([], np.zeros((0, 4), dtype=np.float32))
    _unchanged(pw, before)
    for bad_n in (0, 65, -3):
        with pytest.raises(PhxError) as e:
            pw.pin_iterations = bad_n
        assert e.value.status == ERR_INVALID and pw.pin_iterations == ITERS
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_pins(np.array([good], dtype=pin_dtype)), lambda: pw.remove_pins([0]),
                 lambda: pw.set_pin_anchors([0], np.zeros((1, 4), dtype=np.float32)), lambda: setattr(pw, "pin_iterations", 4), pw.pin_schedule):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.pin_count() == np_ and pw.pin_iterations == ITERS


def test_sharded_worlds_carry_no_pins(built_lib):
    pw = _chain_world(links=3)
    with pytest.raises(PhxError) as e:
        pw.set_shard(0, 2)
    assert e.value.status == ERR_STATE and "pins" in str(e.value)
    n = pw.counts()[0]
    with pytest.raises(PhxError) as e:
        pw.reslab(np.arange(n, dtype=np.int64), n, (-1e9, 1e9))
    assert e.value.status == ERR_STATE and "pins" in str(e.value)
    pw.set_shard(0, 1)
    sharded = phyx_amd.World(0, gravity=G)
    sharded.add_scene(scenes.stack(2, 3))
    sharded.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        sharded.add_pins(_pins([(1, 2, (0.0, 5.0), (0.0, -5.0))]))
    assert e.value.status == ERR_STATE and sharded.pin_count() == 0


def test_set_comm_refuses_a_world_with_pins(built_lib):
    """phx_world_set_comm with a one-rank communicator on a world that holds pins: PHX_ERR_STATE, nothing changed; without pins it attaches,
    and add_pins is then refused.  In a child process, as the other tests that create a communicator: RCCL's bootstrap must not be able
    to hang the suite's process (the library gives up after PHX_COMM_TIMEOUT_S)."""
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pins_comm_worker.py")
    env = dict(os.environ, PHX_COMM_TIMEOUT_S="60")
    for attempt in range(2):
        p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
        if "NO COMMUNICATOR" not in p.stdout:
            break
    if "NO COMMUNICATOR" in p.stdout:
        pytest.skip("no RCCL communicator on this box: " + p.stdout[-300:])
    assert p.returncode == 0 and "pins comm worker ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
