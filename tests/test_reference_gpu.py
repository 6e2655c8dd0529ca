"""The device against the reference's own World / Collider / Solver, with no oracle in the loop (MI355X).

The reference is oracle/_ref/libphyx_ref_full_{strict,fast}.so (oracle/Makefile `ref_full`, ref_harness/full_harness.cpp), built
from the reference's sources where they exist and carried with the tree; these tests read nothing else of the reference, and
skip, saying so, only where those libraries are absent.  The reference steps with 0 workers on its parallel pair path
(UpdatePairsParallel): the path of its threaded configuration, and the one the device restates.

  * non-solver stages, per step: the reference's state after step k is loaded into a device world (phx_world_set_state), both
    step once, and the device's manifolds, contact points and joint topology must equal the reference's byte for byte.  This
    covers IntegrateVelocity, the broadphase, the pair set, the narrowphase, PackManifolds and RefreshContactJoints; the solve is
    order dependent and is pinned through the oracle (test_world_gpu.py, test_reference_lockstep.py).
  * the broadphase at the sizes of test_broadphase_gpu.py against the reference's Collider: sorted entries and entries byte for
    byte, the new pairs element for element in the reference's emission order.
  * the north-star tolerance with band and target taken from the FAST library (the reference's own compiler flags): the twins of
    test_reference_order_tolerance.py's device tests, whose oracle-based originals stay as they are.
"""
import os

import numpy as np
import pytest

import phyx_amd
from phyx_amd import scenes, Configuration
from oracle import binding as ob
import reference_runs as rr
from test_reference_order_tolerance import K_STEPS, ITERS, DT, _check, _diff

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(not os.path.exists(ob.ref_full_path(k)) for k in ob.REF_KINDS),
                                 reason="oracle/_ref/libphyx_ref_full_{strict,fast}.so absent: `make -C oracle ref_full` builds them "
                                        "where the reference's sources are")]


def _ref_world(scene, kind="strict"):
    w = ob.RefWorld(kind, -200.0, ob.PAIRS_PARALLEL)
    w.add_scene(scene)
    return w


def _ref_state(w):
    """The reference world's state as phx_world_set_state takes it: the contact-point slots no manifold owns and the two padding bytes
    of every point zeroed (the reference leaves them unwritten; nothing reads them)."""
    cp = np.zeros_like(w.contact_points())
    m = w.manifolds()
    first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    cp[live] = rr.live_contact_points(w)
    return w.bodies(), m, cp, w.joints()


def _device_live_points(pw):
    m = pw.manifolds
    first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    cp = pw.contactPoints[live].copy()
    cp["pad"] = 0
    return cp


STAGE_SCENES = {"falling1k": (lambda: scenes.falling(1000, width=400.0, ymax=600.0), 200),
                "demo5": (lambda: scenes.reference(5, boxes=360), 120)}


@pytest.mark.parametrize("island_mode", [ob.ISLAND_SINGLE, ob.ISLAND_MULTIPLE_SLOPPY])
@pytest.mark.parametrize("name", list(STAGE_SCENES))
def test_non_solver_stages_match_the_reference_from_its_own_state(built_lib, name, island_mode):
    make, steps = STAGE_SCENES[name]
    rw = _ref_world(make())
    pw = phyx_amd.World(0, gravity=-200.0)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, island_mode, rr.ITERS, rr.ITERS)
    contacts = 0
    for step in range(steps):
        pw.set_state(*_ref_state(rw))                       # the reference's state after `step` steps, warm-start impulses included
        rw.update(DT, ob.SOLVE_AVX2, island_mode, rr.ITERS, rr.ITERS)
        pw.Update(DT, cfg)
        m = rw.manifolds()
        assert pw.counts()[1:] == (len(m), len(rw.contact_points()), len(rw.joints())), "step %d" % step
        assert pw.manifolds.tobytes() == m.tobytes(), "manifolds differ at step %d" % step
        assert _device_live_points(pw).tobytes() == rr.live_contact_points(rw).tobytes(), "contact points differ at step %d" % step
        dj, rj = pw.contactJoints, rw.joints()
        for f in ("contact_point_index", "body1", "body2"):
            assert (dj[f] == rj[f]).all(), "joint %s differ at step %d" % (f, step)
        contacts += len(rj)
    assert contacts > 0


def _ref_collider():
    """A reference harness whose World holds no body: only its Collider is used (full_harness.cpp reff_collider_update)."""
    return ob.RefWorld("strict", -200.0, ob.PAIRS_PARALLEL)


def _check_collider(collider, rw, bodies):
    want_new = rw.collider_update(bodies)
    got_new = collider.UpdateBroadphaseAndPairs(bodies)
    gs, ge = collider.sorted(len(bodies))
    assert gs.tobytes() == rw.broadphase_sorted().tobytes(), "sorted {key,index} sequence differs from the reference's"
    assert ge.tobytes() == rw.broadphase_entries().tobytes(), "BroadphaseEntry records differ from the reference's"
    assert got_new.shape == want_new.shape and (got_new == want_new).all(), "new pairs or their emission order differ from the reference's"
    return got_new


def _random_boxes(rng, n, minx):
    b = np.zeros(n, dtype=phyx_amd.rigid_body_dtype)
    b["aabb_min"]["x"] = minx
    b["aabb_max"]["x"] = minx + rng.uniform(0, 3, n).astype(np.float32)
    b["aabb_min"]["y"] = rng.uniform(-50, 50, n).astype(np.float32)
    b["aabb_max"]["y"] = b["aabb_min"]["y"] + rng.uniform(0, 30, n).astype(np.float32)
    return b


@pytest.mark.parametrize("scene", ["stack2x10", "stack10x100", "falling", "tilted", "wide", "hub"])
def test_broadphase_scenes_match_the_reference_collider(built_lib, scene):
    sc = {"stack2x10": lambda: scenes.stack(2, 10), "stack10x100": lambda: scenes.stack(10, 100),
          "falling": lambda: scenes.falling(3000, width=200.0, ymax=300.0), "tilted": lambda: scenes.tilted(200),
          "wide": lambda: scenes.stack(700, 3), "hub": lambda: scenes.stack(1200, 8)}[scene]()
    rw = _ref_world(sc)
    for _ in range(3):                                      # bodies as the reference's own steps leave them
        rw.update(DT, ob.SOLVE_AVX2, ob.ISLAND_SINGLE, rr.ITERS, rr.ITERS)
    b = rw.bodies()
    assert len(_check_collider(phyx_amd.Collider(0), _ref_collider(), b)) > 0


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 767, 769, 2047, 2048, 2049, 4095, 4097, 12289])
def test_broadphase_edge_sizes_match_the_reference_collider(built_lib, n):
    """Ties, signed zeros, tiny and huge keys, at the sizes where the device's sorts change their bucket counts; three random fills
    each, as test_broadphase_gpu.py draws them."""
    rng = np.random.default_rng(n + 101)
    vals = np.array([-7507.5, -15.0, -0.0, 0.0, 5.0, 20.0, 1e-30, -1e-30, 3e38], dtype=np.float32)
    collider = phyx_amd.Collider(0)
    for rep in range(3):
        collider.clear()
        minx = np.where(rng.random(n) < 0.3, rng.choice(vals, size=n), rng.uniform(-100, 100, n)).astype(np.float32)
        _check_collider(collider, _ref_collider(), _random_boxes(rng, n, minx))


def test_broadphase_1m_boxes_match_the_reference_collider(built_lib):
    """BASELINE config 4's size (1 000 001 bodies, stack(10000, 100)): the whole pair list, element for element; then a second
    update over the same bodies (the two-level sort) reports nothing new, on both sides."""
    sc = scenes.stack(10000, 100)
    rw = _ref_world(sc)
    b = rw.bodies()
    collider = phyx_amd.Collider(0)
    new = _check_collider(collider, rw, b)
    assert len(new) >= 1000000
    assert len(_check_collider(collider, rw, b)) == 0


def _fast_reference(scene, solve_mode, steps):
    w = _ref_world(scene, "fast")
    out = {}
    for k in range(1, max(steps) + 1):
        w.update(DT, solve_mode, ob.ISLAND_SINGLE, ITERS, ITERS)
        if k in steps:
            b = w.bodies()
            out[k] = (b["pos"].copy(), b["velocity"].copy())
    return out


@pytest.mark.parametrize("island_mode", [phyx_amd.ISLAND_SINGLE, phyx_amd.ISLAND_SINGLE_SLOPPY])
def test_device_world_is_within_the_fast_reference_cross_mode_band(built_lib, island_mode):
    """test_device_world_is_within_the_reference_cross_mode_band with the band (Scalar against AVX2) and the target (AVX2) taken from
    the reference built with its own flags (-O3 -ffast-math -mavx2 -mfma) instead of from the oracle."""
    scene = scenes.stack(10, 100)
    scalar = _fast_reference(scene, ob.SOLVE_SCALAR, K_STEPS)
    avx2 = _fast_reference(scene, ob.SOLVE_AVX2, K_STEPS)
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scene)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, island_mode, ITERS, ITERS)
    dev = {}
    for k in range(1, max(K_STEPS) + 1):
        w.Update(DT, cfg)
        if k in K_STEPS:
            b = w.bodies
            dev[k] = (b["pos"].copy(), b["velocity"].copy())
    _check(dev, scalar, avx2)


def test_full_size_200k_boxes_within_the_fast_reference_cross_mode_band(built_lib):
    """test_full_size_200k_boxes_within_the_cross_mode_band against the fast reference library."""
    scene = scenes.stack(1000, 200)
    steps = (1, 2, 3)
    scalar, avx2 = _fast_reference(scene, ob.SOLVE_SCALAR, steps), _fast_reference(scene, ob.SOLVE_AVX2, steps)
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scene)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, ITERS, ITERS)
    for k in range(1, max(steps) + 1):
        w.Update(DT, cfg)
        b = w.bodies
        dev = (b["pos"], b["velocity"])
        band, got = _diff(scalar[k], avx2[k]), _diff(dev, avx2[k])
        print("200k step %d: device-AVX2 %s, band %s" % (k, got, band))
        assert np.isfinite(dev[0]["x"]).all() and np.isfinite(dev[1]["y"]).all()
        assert got[0] <= 2.0 * band[0] + 1e-6 and got[2] <= 2.0 * band[2] + 1e-6, (k, got, band)
        if k == 1:
            assert got[0] <= 1e-3 and got[1] <= 0.1 and got[2] <= 0.05, got
