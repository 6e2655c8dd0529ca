"""Removal of bodies between steps (include/phyx_amd.h, phx_world_remove_bodies / phx_world_remove_outside): what can be checked
without a GPU — the entry points refuse a null handle, the Python wrappers refuse bad input before any C call, and the
specification (tests/removal_spec.py) gives states phx_world_set_state accepts."""
import ctypes as C

import numpy as np
import pytest

import removal_spec
from phyx_amd.api import contact_joint_dtype, contact_point_dtype, manifold_dtype, rigid_body_dtype


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    idx = np.array([0], dtype=np.int32)
    remap = np.zeros(4, dtype=np.int32)
    box = np.array([-1.0, -1.0, 1.0, 1.0], dtype=np.float32)
    removed = C.c_int32(0)
    assert L.phx_world_remove_bodies(None, idx.ctypes.data_as(C.c_void_p), 1, remap.ctypes.data_as(C.c_void_p)) == -1
    assert L.phx_world_remove_bodies(None, None, 0, None) == -1
    assert L.phx_world_remove_outside(None, box.ctypes.data_as(C.c_void_p), C.byref(removed), remap.ctypes.data_as(C.c_void_p)) == -1
    assert L.phx_world_remove_outside(None, None, None, None) == -1
    assert b"null handle" in L.phx_last_error()


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world():
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = _NoC(), None
    return w


def test_remove_bodies_refuses_bad_indices():
    w = _world()
    with pytest.raises(TypeError):
        w.remove_bodies(np.array([0.0, 1.0]))                       # indices must be integers
    with pytest.raises(TypeError):
        w.remove_bodies(np.array([[0, 1]]))                         # ... in a 1-D array
    with pytest.raises(TypeError):
        w.remove_bodies(np.array([True, False]))
    with pytest.raises(TypeError):
        w.remove_bodies(3)
    with pytest.raises(ValueError):
        w.remove_bodies(np.array([0, 2 ** 40]))                     # beyond int32
    with pytest.raises(TypeError):
        w.remove_bodies(np.zeros(0))                                # an empty float array is still a float array


@pytest.mark.parametrize("box", [(0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0, 2.0), np.zeros((2, 2)), ("a", "b", "c", "d"),
                                 (0.0, 0.0, np.nan, 1.0), (0.0, -np.inf, 1.0, 1.0), (0.0, 0.0, 1e39, 1.0),
                                 (2.0, 0.0, 1.0, 1.0), (0.0, 2.0, 1.0, 1.0)])
def test_remove_outside_refuses_bad_boxes(box):
    w = _world()
    with pytest.raises((TypeError, ValueError)):
        w.remove_outside(box)


def _records(n):
    b = np.zeros(n, dtype=rigid_body_dtype)
    b["index"] = np.arange(n, dtype=np.uint32)
    b["pos"]["x"] = np.arange(n, dtype=np.float32) * 10.0
    b["velocity"]["y"] = -np.arange(n, dtype=np.float32)
    b["acceleration"]["x"][n // 2] = 3.0
    b["aabb_min"]["x"] = b["pos"]["x"] - 5.0
    b["aabb_max"]["x"] = b["pos"]["x"] + 5.0
    b["aabb_min"]["y"] = -5.0
    b["aabb_max"]["y"] = 5.0
    return b


def _state(bodies, manifolds, slots, joints):
    m = np.zeros(len(manifolds), dtype=manifold_dtype)
    for i, (b1, b2, pc) in enumerate(manifolds):
        m[i] = (b1, b2, pc, 2 * i)
    cps = np.zeros(2 * len(manifolds), dtype=contact_point_dtype)
    cps["solver_index"] = slots
    cps["normal"]["y"] = np.arange(len(cps), dtype=np.float32)
    j = np.zeros(len(joints), dtype=contact_joint_dtype)
    for k, c in enumerate(joints):
        j[k] = (c, m[c // 2]["body1"], m[c // 2]["body2"], 1.0 + k, -0.5 * k)
    return bodies, m, cps, j


def test_worked_example():
    """Five bodies, body 2 removed: manifolds (0,1) x2 points, (1,2) x1, (0,3) x1, (2,4) dead; joints on slots 0, 2, 1, 4."""
    st = _state(_records(5), [(0, 1, 2), (1, 2, 1), (0, 3, 1), (2, 4, 0)], [0, 2, 1, -1, 3, 7, -1, 5], [0, 2, 1, 4])
    assert removal_spec.set_state_problems(st) == []
    (b, m, c, j), new = removal_spec.filter(st, [2])
    assert new.tolist() == [0, 1, -1, 2, 3]
    assert b["index"].tolist() == [0, 1, 2, 3]
    assert b["pos"]["x"].tolist() == [0.0, 10.0, 30.0, 40.0]
    assert b["acceleration"]["x"].tolist() == [0.0, 0.0, 0.0, 0.0]              # body 2 took its acceleration along
    assert m.tolist() == [(0, 1, 2, 0), (0, 2, 1, 2)]
    assert c["solver_index"].tolist() == [0, 1, 2, 7]                          # live slots follow their joints; the dead slot is copied
    assert c["normal"]["y"].tolist() == [0.0, 1.0, 4.0, 5.0]
    assert j[["contact_point_index", "body1", "body2"]].tolist() == [(0, 0, 1), (1, 0, 1), (2, 0, 2)]
    assert j["normal_acc"].tolist() == [1.0, 3.0, 4.0]                         # warm-start impulses unchanged
    assert removal_spec.set_state_problems((b, m, c, j)) == []


def test_worked_example_removals_at_the_edges():
    st = _state(_records(5), [(0, 1, 2), (1, 2, 1), (0, 3, 1), (2, 4, 0)], [0, 2, 1, -1, 3, 7, -1, 5], [0, 2, 1, 4])
    (b, m, c, j), new = removal_spec.filter(st, [])
    assert all(x.tobytes() == y.tobytes() for x, y in zip((b, m, c, j), st)) and new.tolist() == list(range(5))
    (b, m, c, j), new = removal_spec.filter(st, [4, 0, 1, 2, 3])
    assert (len(b), len(m), len(c), len(j)) == (0, 0, 0, 0) and (new == -1).all()
    (b, m, c, j), new = removal_spec.filter(st, [0])                           # the ground: only (1,2) and (2,4) stay
    assert m.tolist() == [(0, 1, 1, 0), (1, 3, 0, 2)]
    assert j[["contact_point_index", "body1", "body2"]].tolist() == [(0, 0, 1)]
    assert c["solver_index"].tolist() == [0, -1, -1, 5]
    assert removal_spec.set_state_problems((b, m, c, j)) == []


def _random_state(rng, nb):
    """A state as a world leaves it between steps: manifolds on distinct pairs b1 < b2, live slots with joints in a shuffled order."""
    bodies = _records(nb)
    pairs = set()
    while len(pairs) < min(3 * nb, nb * (nb - 1) // 2):
        a, b = sorted(rng.choice(nb, size=2, replace=False).tolist())
        pairs.add((a, b))
    pairs = list(pairs)
    rng.shuffle(pairs)
    manifolds = [(a, b, int(rng.integers(0, 3))) for a, b in pairs]
    live = [2 * i + k for i, (_, _, pc) in enumerate(manifolds) for k in range(pc)]
    order = rng.permutation(len(live))
    joints = [live[o] for o in order]
    slots = rng.integers(-1, 50, size=2 * len(manifolds))
    for jj, c in enumerate(joints):
        slots[c] = jj
    return _state(bodies, manifolds, slots.astype(np.int32), joints)


@pytest.mark.parametrize("seed", range(12))
def test_random_states_stay_acceptable(seed):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(2, 40))
    st = _random_state(rng, nb)
    assert removal_spec.set_state_problems(st) == []
    removed = rng.choice(nb, size=int(rng.integers(0, nb + 1)), replace=False)
    (b, m, c, j), new = removal_spec.filter(st, removed)
    assert removal_spec.set_state_problems((b, m, c, j)) == []
    keep = np.ones(nb, dtype=bool)
    keep[removed] = False
    want = st[0][keep].copy()
    want["index"] = np.arange(len(want), dtype=np.uint32)
    assert b.tobytes() == want.tobytes()                                        # records unchanged but for their index
    mk = keep[st[1]["body1"]] & keep[st[1]["body2"]]
    assert len(m) == mk.sum() and (m["point_count"] == st[1]["point_count"][mk]).all()
    assert (m["body1"] < m["body2"]).all()
    assert len(j) == int(m["point_count"].sum())                                # a joint per live slot of the kept manifolds
    assert (j["normal_acc"] == st[3]["normal_acc"][mk[st[3]["contact_point_index"] // 2]]).all()
    assert (new[keep] == np.arange(keep.sum())).all() and (new[~keep] == -1).all()


def test_outside_is_the_closed_box():
    b = _records(6)                                                             # AABBs [10 i - 5, 10 i + 5] x [-5, 5]
    assert removal_spec.outside(b, (15.0, -5.0, 25.0, 5.0)).tolist() == [0, 4, 5]       # touching edges overlap
    assert removal_spec.outside(b, (15.0, 5.5, 25.0, 9.0)).tolist() == [0, 1, 2, 3, 4, 5]
