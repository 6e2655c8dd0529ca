"""Force fields on the device (phx_world_set_fields / pulse_fields / apply_impulses), byte for byte against tests/field_spec.py: before
every step the oracle World's acceleration fields are set to the spec's sums (pending + the fields, as test_body_edits_gpu's
_oracle_add_accel bumps them), then both worlds step in lockstep (spawn_lockstep) and every byte is compared."""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, scenes, uniform_field, radial_field, drag_field, field_dtype
from phyx_amd.api import frame_from_angle, _lib
from helpers import oracle_world, oracle_set_pose, oracle_set_velocity
import field_spec
import pin_spec
import spawn_lockstep

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
F = np.float32
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)


def _grid(n, pitch=30.0, columns=32):
    """n free boxes of half-size 5 on a grid, far enough apart never to touch; no ground"""
    k = np.arange(n)
    return scenes._scene((k % columns) * pitch, 100.0 + (k // columns) * pitch, np.zeros(n), np.full(n, 5.0), np.full(n, 5.0), np.zeros(n, dtype=bool))


def _worlds(scene, timing=False):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scene)
    if timing:
        pw.set_phase_timing(True)
    return pw, oracle_world(scene)


def _categories(pw):
    f = pw.collision_filters()
    return None if (f["category"] == 1).all() and (f["mask"] == 0xFFFFFFFF).all() else f["category"]


def _bump(ow, fields, dt, categories=None):
    """the oracle's acceleration fields become the spec's sums: what the device's pass leaves for IntegrateVelocity"""
    b = ow.bodies()
    if not len(fields):
        return 0
    a = field_spec.step_accelerations(fields, dt, b, categories)
    acted = int((a != field_spec.pending_of(b)).any(axis=1).sum())
    b["acceleration"]["x"][:], b["acceleration"]["y"][:], b["angular_acceleration"][:] = a[:, 0], a[:, 1], a[:, 2]
    return acted                                            # how many bodies the fields reached


def _step(oracle, pw, ow, cfg=CFG, dt=DT, categories=None):
    acted = _bump(ow, pw.fields(), dt, categories)
    spawn_lockstep.step(oracle, pw, ow, cfg, dt)
    return acted


def _stack(fields):
    return np.stack(fields) if len(fields) else np.zeros(0, dtype=field_dtype)


def _mixed_fields(count, drag, masked, extent):
    """`count` fields of every kind and shape over a grid of width `extent`; a DRAG among them iff `drag`; masks that hit and miss
    category 1 iff `masked` (else all-ones)"""
    rng = np.random.default_rng(count * 4 + drag * 2 + masked)
    out = []
    for k in range(count):
        c = rng.uniform(0.0, extent, 2) + (0.0, 100.0)
        region = [{}, {"box": (c[0] - 70.0, c[1] - 40.0, c[0] + 70.0, c[1] + 40.0)}, {"disc": (c[0], c[1], rng.uniform(20.0, 200.0))}][k % 3]
        mask = [5, 6, 0xFFFFFFFF, 1][k % 4] if masked else 0xFFFFFFFF
        kind = (2 + k + k // 3) % 3 if drag else (k // 3) % 2          # (against the shape's k % 3: every kind meets every shape)
        force = bool((k // 9) % 2)
        if kind == 0:
            out.append(uniform_field(*rng.uniform(-50.0, 50.0, 3), mask=mask, force=force, **region))
        elif kind == 1:
            out.append(radial_field(c[0] + 3.0, c[1] - 7.0, rng.uniform(-200.0, 200.0), [0.0, 150.0][k % 2], mask=mask, force=force, **region))
        else:
            out.append(drag_field(rng.uniform(0.0, 90.0), rng.uniform(0.0, 90.0), flow=rng.uniform(-20.0, 20.0, 2), mask=mask, force=force, **region))
    f = _stack(out)
    assert (f["kind"] == 2).any() == bool(drag)
    return f


def _one_step_both_ways(oracle, n, fields):
    """one step of n free bodies under `fields`, fused and under phase timing (the unfused IntegrateVelocity), against one oracle step"""
    scene = _grid(n)
    rng = np.random.default_rng(n)
    vel = rng.uniform(-30.0, 30.0, (n, 3)).astype(np.float32)
    ow = None
    for timing in (False, True):
        pw, o = _worlds(scene, timing)
        pw.set_fields(fields)
        pw.set_velocities(np.arange(n), vel)
        assert pw.field_passes() == 0
        if ow is None:
            ow = o
            for i in range(n):
                oracle_set_velocity(ow, i, vel[i])
            b = ow.bodies()
            want = field_spec.step_accelerations(fields, DT, b)
            assert want.any(), "the fields reach no body: the case checks nothing"
            b["acceleration"]["x"][:], b["acceleration"]["y"][:], b["angular_acceleration"][:] = want[:, 0], want[:, 1], want[:, 2]
            spawn_lockstep.step(oracle, pw, ow, CFG, DT)
        else:
            pw.Update(DT, CFG)
        assert pw.field_passes() == 1
        spawn_lockstep.compare(pw, ow, 0)
        b = pw.bodies
        v = field_spec.velocities_of(b)
        gravity = np.where(b["inv_mass"] > 0, F(G), F(0))
        expect = np.stack([vel[:, 0] + want[:, 0] * F(DT), vel[:, 1] + (want[:, 1] + gravity) * F(DT), vel[:, 2] + want[:, 2] * F(DT)], axis=1)
        assert v.tobytes() == expect.astype(np.float32).tobytes()
        assert not field_spec.pending_of(b).any()


# ---- 1. edges of the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_body_counts_around_the_wave_and_the_workgroup(oracle, built_lib, n):
    k = [1, 63, 64, 65, 255, 256, 257, 1025].index(n)
    _one_step_both_ways(oracle, n, _mixed_fields(2 if n > 1 else 1, drag=k & 1, masked=(k >> 1) & 1, extent=30.0 * min(n, 32)))


@pytest.mark.parametrize("count", [1, 2, 64, 256])
@pytest.mark.parametrize("drag", [0, 1])
@pytest.mark.parametrize("masked", [0, 1])
def test_field_counts_and_every_instance(oracle, built_lib, count, drag, masked):
    _one_step_both_ways(oracle, 65, _mixed_fields(count, drag, masked, extent=960.0))


# ---- 2. edges of the rules ----------------------------------------------------------------------------------------------------------------
def _up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def test_edges_of_the_rules(oracle, built_lib):
    names = ["box edge", "past the box edge", "disc rim", "past the disc rim", "radial centre", "at the falloff radius", "inside the falloff",
             "radius 0 disc", "static", "no inertia", "category 4 a", "category 4 b", "elsewhere"]
    at = {n: i for i, n in enumerate(names)}
    pw, ow = _worlds(_grid(len(names), pitch=40.0, columns=4))
    place = {"box edge": (1100.0, 1010.0), "past the box edge": (_up(1100.0), 1040.0), "disc rim": (2250.0, 2000.0), "past the disc rim": (2000.0, _up(2250.0)),
             "radial centre": (3000.0, 3000.0), "at the falloff radius": (4064.0, 4000.0), "inside the falloff": (4000.0, 4032.0), "radius 0 disc": (5000.0, 5000.0)}
    idx = [at[n] for n in place]
    poses = np.stack([frame_from_angle(x, y, 0.0) for x, y in place.values()])
    pw.set_poses(idx, poses)
    for i, p in zip(idx, poses):
        oracle_set_pose(oracle, ow, i, p)
    pw.set_inverse_masses([at["static"], at["no inertia"]], np.array([[0.0, 0.0], [2.0, 0.0]], dtype=np.float32))
    b = ow.bodies()
    b["inv_mass"][at["static"]], b["inv_inertia"][at["static"]] = 0.0, 0.0
    b["inv_mass"][at["no inertia"]], b["inv_inertia"][at["no inertia"]] = 2.0, 0.0
    fields = _stack([
        uniform_field(10.0, 0.0, box=(1000.0, 1000.0, 1100.0, 1050.0)),                       # 0
        uniform_field(0.0, 20.0, disc=(2000.0, 2000.0, 250.0)),                               # 1
        radial_field(3000.0, 3000.0, 500.0, disc=(3000.0, 3000.0, 10.0)),                     # 2: d = 0 at its centre
        radial_field(4000.0, 4000.0, -300.0, 64.0, disc=(4000.0, 4000.0, 100.0)),             # 3: t = 0 at d = 64
        uniform_field(0.0, 0.0, 7.0, disc=(5000.0, 5000.0, 0.0)),                             # 4: a disc of radius 0 holds its centre
        uniform_field(3.0, 0.0, 5.0, force=True),                                             # 5: ALL, scaled by the inverse masses
        uniform_field(0.0, 0.0, 11.0, mask=6),                                                # 6: misses category 1
    ])
    pw.set_fields(fields)
    want = field_spec.step_accelerations(fields, DT, ow.bodies())
    base = field_spec.step_accelerations(fields[5:6], DT, ow.bodies())                        # what the ALL field alone gives everybody
    touched = {n for n in names if want[at[n]].tobytes() != base[at[n]].tobytes()}
    assert touched == {"box edge", "disc rim", "inside the falloff", "radius 0 disc"}, touched
    assert not want[at["static"]].any()
    im = F(ow.bodies()["inv_mass"][at["no inertia"]])
    assert want[at["no inertia"]].tolist() == [F(3.0) * im, 0.0, 0.0]
    _step(oracle, pw, ow)
    spawn_lockstep.compare(pw, ow, 0)
    # the filter column appears: two bodies get category 4, which mask 6 hits
    cat4 = [at["category 4 a"], at["category 4 b"]]
    pw.set_collision_filters(cat4, category=4)
    cats = _categories(pw)
    assert cats is not None and cats[cat4].tolist() == [4, 4]
    want = field_spec.step_accelerations(fields, DT, ow.bodies(), cats)
    assert [bool(want[i, 2] != base[i, 2]) for i in range(len(names))] == [i in cat4 for i in range(len(names))]      # (the step moved the body off the radius 0 disc)
    _step(oracle, pw, ow, categories=cats)
    spawn_lockstep.compare(pw, ow, 1)
    # a category of 0 passes no mask, all-ones included
    pw.set_collision_filters([at["elsewhere"]], category=0)
    cats = _categories(pw)
    assert not field_spec.step_accelerations(fields, DT, ow.bodies(), cats)[at["elsewhere"]].any()
    _step(oracle, pw, ow, categories=cats)
    spawn_lockstep.compare(pw, ow, 2)


def test_a_nan_position_is_outside_every_shape_but_all(built_lib):
    """Through the pulse, which is the same device body with the velocity as destination: a body without a position is not put through
    a step's broadphase for this."""
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(_grid(3))
    pose = frame_from_angle(0.0, 0.0, 0.0)
    pose[0] = np.nan
    pw.set_poses([1], pose[None, :])
    fields = _stack([uniform_field(1.0, 0.0, box=(-1e9, -1e9, 1e9, 1e9)), uniform_field(0.0, 2.0, disc=(0.0, 0.0, 1e9)),
                     radial_field(5.0, 5.0, 9.0), drag_field(0.5, 0.5, flow=(8.0, 8.0)), uniform_field(0.0, 0.0, 4.0)])
    before = pw.bodies
    want = field_spec.pulse(fields, before)
    assert want[1].tolist() == [4.0, 4.0, 4.0] and want[0, 0] != 4.0          # the drag and the last field only: both ALL, neither reads the position
    pw.pulse_fields(fields)
    assert field_spec.velocities_of(pw.bodies).tobytes() == want.tobytes()


# ---- 3. the order of the sum ------------------------------------------------------------------------------------------------------------
def test_pending_then_the_fields_in_list_order(oracle, built_lib):
    pw, ow = _worlds(_grid(6))
    fields = _stack([uniform_field(1.0, 0.25, 0.5), uniform_field(2.0 ** 25, 0.0), uniform_field(-(2.0 ** 25), 3.0)])      # 0 + 1 + 2^25 - 2^25 = 0,
    other = fields[[1, 2, 0]]                                                                                              # 0 + 2^25 - 2^25 + 1 = 1
    pw.set_fields(fields)
    pending = np.array([[-(2.0 ** 25), 1.0, 2.0], [3.0, 0.1, 0.7], [1e-3, -5.0, 0.0]], dtype=np.float32)
    for round_ in range(2):                                 # with something pending on three bodies, then with nothing pending
        if round_ == 0:
            pw.add_accelerations([0, 2, 4], pending)
            b = ow.bodies()
            for i, a in zip([0, 2, 4], pending):
                b["acceleration"]["x"][i] += a[0]; b["acceleration"]["y"][i] += a[1]; b["angular_acceleration"][i] += a[2]
        want = field_spec.step_accelerations(fields, DT, ow.bodies())
        assert want.tobytes() != field_spec.step_accelerations(other, DT, ow.bodies()).tobytes(), "the order does not show in these values"
        _step(oracle, pw, ow)
        spawn_lockstep.compare(pw, ow, round_)
        assert not field_spec.pending_of(pw.bodies).any()


# ---- 4. lockstep with contacts ----------------------------------------------------------------------------------------------------------
def _stack_and_free_boxes():
    s = scenes.stack(4, 12)
    k = np.arange(8)
    free = scenes._scene(100.0 + 30.0 * k, 200.0 + 10.0 * (k % 2), 0.1 * k, np.full(8, 5.0), np.full(8, 4.0), np.zeros(8, dtype=bool))
    return {key: np.concatenate([s[key], free[key]]) for key in s}


@pytest.mark.parametrize("island_mode", [phyx_amd.ISLAND_SINGLE, phyx_amd.ISLAND_MULTIPLE_SLOPPY])
def test_lockstep_with_a_wind_a_pool_and_an_attractor(oracle, built_lib, island_mode):
    cfg = Configuration(phyx_amd.SOLVE_AVX2, island_mode, 15, 15)
    pw, ow = _worlds(_stack_and_free_boxes())
    first = _stack([uniform_field(90.0, 0.0, box=(-40.0, 95.0, 25.0, 160.0)),                       # a wind across the stack's top
                    drag_field(4.0, 2.0, box=(-45.0, 10.0, 30.0, 45.0)),                            # a pool at the ground
                    radial_field(200.0, 150.0, -400.0, 220.0, disc=(200.0, 150.0, 200.0))])         # an attractor over the free boxes
    second = _stack([radial_field(0.0, 60.0, 250.0, 90.0, force=False), uniform_field(0.0, 3.0e-3, 1.0e-4, force=True, disc=(200.0, 150.0, 300.0)),
                     drag_field(30.0, 90.0, flow=(-15.0, 0.0), box=(-100.0, 0.0, 100.0, 200.0)), first[0]])
    pw.set_fields(first)
    for step in range(40):
        if step == 20:
            pw.set_fields(second)
        if step == 30:
            pw.set_fields([])
        assert len(pw.fields()) == [3, 4, 0][(step >= 20) + (step >= 30)]
        acted = _step(oracle, pw, ow, cfg)
        assert (acted >= 8) == (step < 30), "step %d: the fields reached %d bodies" % (step, acted)
        spawn_lockstep.compare(pw, ow, step)
    assert len(ow.joints()) > 0
    assert pw.field_passes() == 30


# ---- 5. no fields, no cost ----------------------------------------------------------------------------------------------------------------
def test_an_empty_list_costs_nothing(built_lib):
    def run(call):
        pw = phyx_amd.World(0, gravity=G)
        pw.add_scene(scenes.stack(4, 12))
        if call:
            pw.set_fields([])
        for _ in range(10):
            pw.Update(DT, CFG)
        return pw

    a, b = run(True), run(False)
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.field_passes() == 0 and b.field_passes() == 0
    assert a.build_counts() == b.build_counts()
    a.set_fields([uniform_field(1.0, 0.0)] * 7)
    for s in range(5):
        a.Update(DT, CFG)
        assert a.field_passes() == s + 1                    # one launch per step, whatever the list's length


def test_set_fields_keeps_the_schedule(built_lib):
    """As test_body_edits_gpu's schedule test: ten steps with the list replaced before each (a wind that only an isolated body stands in)
    rebuild and reuse the schedule exactly as ten steps without."""
    def run(edit):
        pw = phyx_amd.World(0, gravity=G)
        pw.add_scene(scenes.stack(4, 12))
        lone = pw.AddBody((5000.0, 600.0), 0.0, (5.0, 5.0))
        for _ in range(40):                                 # settle
            pw.Update(DT, CFG)
        counts0 = pw.build_counts()
        reuse = []
        for s in range(10):
            if edit:
                pw.set_fields([uniform_field(500.0 + s, -G, box=(4000.0, -1e6, 1e6, 1e6))])
            pw.Update(DT, CFG)
            st = pw.solver.stats()
            reuse.append((st.recoloured, st.graph_replay, st.colour_count, st.island_count))
        counts1 = pw.build_counts()
        b = pw.bodies
        return (counts1[0] - counts0[0], counts1[1] - counts0[1]), reuse, b[:lone].tobytes(), b[lone]

    plain, blown = run(False), run(True)
    assert blown[0] == plain[0] and blown[1] == plain[1]
    assert blown[2] == plain[2]
    assert blown[3]["pos"]["x"] > plain[3]["pos"]["x"] + 1.0


# ---- 6. bookkeeping ---------------------------------------------------------------------------------------------------------------------
def _oracle_from(pw):
    """An oracle World whose records are the device's (a world without contacts carries nothing else from step to step)."""
    assert pw.counts()[1:] == (0, 0, 0)
    b = pw.bodies
    ow = oracle_world(_grid(len(b)))
    ow.bodies().view(np.uint8)[:] = b.view(np.uint8)
    return ow


def test_the_list_survives_what_names_no_field(oracle, built_lib):
    pw, ow = _worlds(_grid(12))
    fields = _stack([uniform_field(30.0, 0.0, 0.2, box=(-10.0, -1e5, 200.0, 1e5)), drag_field(2.0, 1.0, flow=(0.0, -50.0)), radial_field(150.0, 0.0, -80.0, 900.0)])
    pw.set_fields(fields)
    step = [0]

    def five(ow):
        assert pw.fields().tobytes() == fields.tobytes()
        for _ in range(5):
            assert _step(oracle, pw, ow) == len(ow.bodies())
            spawn_lockstep.compare(pw, ow, step[0])
            step[0] += 1

    five(ow)
    pw.remove_bodies([2, 7])
    ow = _oracle_from(pw)
    five(ow)
    new = pw.add_bodies(np.array([[60.0, 400.0, 0.3, 5.0, 4.0]], dtype=np.float32))
    assert ow.add_body(60.0, 400.0, 0.3, 5.0, 4.0) == new[0]
    five(ow)
    snap = pw.save()
    saved = pw.bodies
    five(ow)
    pw.set_state(*pw.state())
    five(ow)
    pw.load(snap)
    assert pw.bodies.tobytes() == saved.tobytes()
    ow = _oracle_from(pw)
    five(ow)
    assert pw.field_passes() == step[0] == 30


def test_refusals(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(_grid(4))
    fields = _stack([uniform_field(1.0, 2.0), radial_field(0.0, 0.0, 5.0, 10.0)])
    pw.set_fields(fields)
    bad = fields.copy()
    bad["mask"][1] = 0
    for call in (pw.set_fields, pw.pulse_fields):
        with pytest.raises(phyx_amd.PhxError) as e:
            call(bad)
        assert e.value.status == _lib.PHX_ERR_INVALID and "field 1: mask 0" in str(e.value)
    assert pw.fields().tobytes() == fields.tobytes()        # an invalid list leaves the old one
    pw.Update(DT, CFG)
    pw.PreSolve(DT)
    for call in (lambda: pw.set_fields([]), lambda: pw.pulse_fields(fields), lambda: pw.apply_impulses([1], np.ones((1, 4), dtype=np.float32))):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == _lib.PHX_ERR_STATE
    pw.FinishStep(DT, CFG)
    assert pw.fields().tobytes() == fields.tobytes()
    with pytest.raises(phyx_amd.PhxError) as e:             # a world with fields does not become a sharded one
        pw.set_shard(0, 2)
    assert e.value.status == _lib.PHX_ERR_STATE and "force fields" in str(e.value)
    pw.set_fields([])
    pw.set_shard(0, 2)                                      # ... and a sharded one takes none
    for call in (lambda: pw.set_fields(fields), lambda: pw.pulse_fields(fields)):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == _lib.PHX_ERR_STATE
    assert len(pw.fields()) == 0
    n = pw.counts()[0]
    one = np.ones((1, 4), dtype=np.float32)
    for idx, vals in (([1, 1], np.ones((2, 4), dtype=np.float32)), ([n], one), ([-1], one), ([0], np.array([[np.nan, 0, 0, 0]], dtype=np.float32))):
        with pytest.raises(phyx_amd.PhxError) as e:
            pw.apply_impulses(idx, vals)
        assert e.value.status == _lib.PHX_ERR_INVALID


# ---- 7. pulses and impulses -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepped", [False, True], ids=["host-staged", "after a step"])
@pytest.mark.parametrize("which", ["blast", "uniform + drag"])
def test_pulse(built_lib, which, stepped):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(_grid(40, columns=8))
    pw.set_inverse_masses([5], np.zeros((1, 2), dtype=np.float32))
    vel = np.random.default_rng(5).uniform(-20.0, 20.0, (40, 3)).astype(np.float32)
    if stepped:
        pw.Update(DT, CFG)
    pw.set_velocities(np.arange(40), vel)
    pw.set_velocities([5], np.zeros((1, 3), dtype=np.float32))
    fields = _stack([radial_field(100.0, 160.0, 900.0, 120.0)] if which == "blast" else
                    [uniform_field(2.0 ** 20, 0.0, 1.0, box=(0.0, 0.0, 100.0, 1e4)), drag_field(0.25, 0.5, flow=(3.0, -1.0))])
    before = pw.bodies
    want = field_spec.pulse(fields, before)
    changed = (want != field_spec.velocities_of(before)).any(axis=1)
    assert changed.any() and not changed[5] and (which != "blast" or not changed.all())         # the static body and the bodies out of range stay
    pw.pulse_fields(fields)
    after = pw.bodies
    assert field_spec.velocities_of(after).tobytes() == want.tobytes()
    assert not field_spec.pending_of(after).any()
    untouched = before.copy()
    for name in ("velocity", "angular_velocity"):
        untouched[name] = after[name]
    assert untouched.tobytes() == after.tobytes()          # nothing but the velocities changed
    assert pw.field_passes() == 0


@pytest.mark.parametrize("stepped", [False, True], ids=["host-staged", "after a step"])
def test_apply_impulses(built_lib, stepped):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(_grid(8))
    pw.set_inverse_masses([3], np.zeros((1, 2), dtype=np.float32))
    if stepped:
        pw.Update(DT, CFG)
    pw.set_velocities([0, 1, 2], np.array([[1.0, 2.0, 0.5], [-3.0, 0.0, 0.25], [0.0, 0.0, 0.0]], dtype=np.float32))
    before = pw.bodies
    pos = np.stack([before["pos"]["x"], before["pos"]["y"]], axis=1)
    imp = np.array([[1e-3, -2e-3, pos[0, 0], pos[0, 1]],                       # through the centre
                    [0.0, 4e-3, pos[1, 0] + 3.0, pos[1, 1] - 1.0],             # off centre
                    [-2e-3, 1e-3, pos[2, 0] - 2.5, pos[2, 1] + 4.0],
                    [5e-3, 5e-3, pos[3, 0] + 1.0, pos[3, 1]]], dtype=np.float32)        # on the static body
    pw.apply_impulses([0, 1, 2, 3], imp)
    after = pw.bodies
    got = field_spec.velocities_of(after)
    for k in range(4):
        assert tuple(got[k]) == field_spec.impulse(before[k], *imp[k]), k
    assert got[0, 2] == before["angular_velocity"][0]       # through the centre: no turn
    assert got[1, 2] < before["angular_velocity"][1]        # r = (3, -1), J = (0, +): counter-clockwise, and the engine's w is clockwise-positive
    assert got[3].tolist() == [0.0, 0.0, 0.0]
    assert got[4:].tobytes() == field_spec.velocities_of(before)[4:].tobytes()
    # the same impulse as a pin would apply it to its second body (pin_spec.apply)
    ref = before.copy()
    for k in range(3):
        p = pin_spec._Pin()
        p.a, p.b, p.write_a, p.write_b = -1, k, False, True
        p.mb, p.ib = F(before["inv_mass"][k]), F(before["inv_inertia"][k])
        p.rbx, p.rby = F(imp[k, 2]) - F(pos[k, 0]), F(imp[k, 3]) - F(pos[k, 1])
        pin_spec.apply(ref, p, F(imp[k, 0]), F(imp[k, 1]))
    assert field_spec.velocities_of(ref)[:3].tobytes() == got[:3].tobytes()


def test_sleepers_are_not_affected_until_they_are_woken(built_lib):
    """A sleeper rests as a static body on the device (inv_mass 0): neither a pulse nor the step's pass writes it, and the pile sleeps on."""
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 2))
    pw.set_sleeping(0.5, 0.05, 0.2)
    for _ in range(300):
        pw.Update(DT, CFG)
        if pw.sleep_counts()[0] == 4:
            break
    assert pw.sleep_counts()[0] == 4, "the pile never came to rest: the test's premise"
    before = pw.bodies
    blast = [radial_field(0.0, 0.0, 500.0, 300.0)]
    pw.pulse_fields(blast)
    assert pw.bodies.tobytes() == before.tobytes()
    pw.set_fields([uniform_field(100.0, 0.0)])
    pw.Update(DT, CFG)
    assert pw.bodies.tobytes() == before.tobytes() and pw.sleep_counts()[0] == 4 and pw.field_passes() == 1
    pw.set_fields([])
    pw.wake_bodies([1, 2, 3, 4])
    want = field_spec.pulse(_stack(blast), pw.bodies)
    pw.pulse_fields(blast)
    got = field_spec.velocities_of(pw.bodies)
    assert got.tobytes() == want.tobytes() and (got[1:] != 0).any(axis=1).all() and not got[0].any()


# ---- 8. behaviour -----------------------------------------------------------------------------------------------------------------------
def test_a_wind_zone_speeds_a_box_up_and_lets_it_keep_its_speed(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.AddBody((0.0, 0.0), 0.0, (2000.0, 10.0), static=True)
    box = pw.AddBody((0.0, 15.0), 0.0, (5.0, 5.0))
    pw.set_materials([0, box], friction=0.0)
    pw.set_fields([uniform_field(300.0, 0.0, box=(-50.0, 0.0, 50.0, 100.0))])
    speeds, xs = [], []
    for _ in range(90):
        pw.Update(DT, CFG)
        b = pw.body_states([box])
        speeds.append(float(b["velocity"]["x"][0])); xs.append(float(b["pos"]["x"][0]))
    inside = [s for s, x in zip(speeds, xs) if x <= 50.0]
    outside = [s for s, x in zip(speeds, xs) if x > 50.0 + 5.0]
    assert len(inside) > 10 and len(outside) > 10
    assert all(b > a for a, b in zip(inside, inside[1:]))
    assert outside[-1] == pytest.approx(outside[0], rel=1e-3) and outside[0] >= inside[-1]


def test_a_drag_pool_halves_the_speed_in_a_step(built_lib):
    pw = phyx_amd.World(0, gravity=0.0)
    pw.add_scene(_grid(2))
    dt = 1.0 / 64.0
    pw.set_velocities([0, 1], np.array([[0.0, -64.0, 2.0], [0.0, -64.0, 2.0]], dtype=np.float32))
    pw.set_fields([drag_field(32.0, 32.0, box=(-10.0, 0.0, 10.0, 1000.0))])          # k dt = 0.5; body 1 is outside
    pw.Update(dt, CFG)
    b = pw.bodies
    assert (b["velocity"]["y"][0], b["angular_velocity"][0]) == (-32.0, 1.0)
    assert (b["velocity"]["y"][1], b["angular_velocity"][1]) == (-64.0, 2.0)


def test_a_blast_scatters_a_ring(built_lib):
    t = 2.0 * np.pi * np.arange(16) / 16.0
    ring = scenes._scene(300.0 + 80.0 * np.cos(t), 300.0 + 80.0 * np.sin(t), np.zeros(16), np.full(16, 5.0), np.full(16, 5.0), np.zeros(16, dtype=bool))
    pw = phyx_amd.World(0, gravity=0.0)
    pw.add_scene(ring)
    pw.pulse_fields([radial_field(300.0, 300.0, 120.0, 200.0)])
    for _ in range(5):
        pw.Update(DT, CFG)
    b = pw.bodies
    out = (b["pos"]["x"] - 300.0) * np.cos(t) + (b["pos"]["y"] - 300.0) * np.sin(t)
    assert (out > 80.0 + 1.0).all()
    radial = b["velocity"]["x"] * np.cos(t) + b["velocity"]["y"] * np.sin(t)
    assert (radial > 0).all()
