"""Collision filters (include/phyx_amd.h, COLLISION FILTERS) without a GPU: the rule's truth table, worked and random examples of
filter_spec.drop, the entry points refuse a null handle, the Python wrapper refuses bad input before any C call, and the record is
12 bytes on both sides of the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_spec as spec
import removal_spec
from phyx_amd.api import collision_filter_dtype, contact_joint_dtype, contact_point_dtype, manifold_dtype, rigid_body_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 0xFFFFFFFF


def _f(category, mask, group):
    return np.array([(category, mask, group)], dtype=collision_filter_dtype)[0]


# (a, b, collide)
TRUTH = [
    ((1, ALL, 0), (1, ALL, 0), True),               # the default passes everything
    ((1, ALL, 3), (1, ALL, 3), True),               # a shared positive group
    ((1, 0, 3), (2, 0, 3), True),                   # ... overrides masks that would reject
    ((1, ALL, -2), (1, ALL, -2), False),            # a shared negative group never collides
    ((1, ALL, -2), (1, ALL, 2), True),              # different groups: the masks decide
    ((1, ALL, -2), (1, ALL, -3), True),
    ((1, 0, -2), (1, ALL, -3), False),
    ((1, ALL, 0), (1, ALL, 5), True),               # group 0 is no group
    ((1, 0, 0), (1, 0, 0), False),                  # group 0 shared is no shared group: masks 0 reject
    ((1, 0, 0), (1, ALL, 0), False),                # mask 0: collides with nothing (a ghost)
    ((1, ALL, 0), (1, 0, 0), False),
    ((0, ALL, 0), (1, ALL, 0), False),              # category 0: nothing's mask meets it
    ((1, ALL, 0), (0, ALL, 0), False),
    ((0, ALL, 7), (0, ALL, 7), True),               # ... unless a shared positive group decides
    ((2, 2, 0), (1, ALL, 0), False),                # layer 2 only with layer 2
    ((2, 2, 0), (2, 2, 0), True),
    ((2, 3, 0), (1, 2, 0), True),                   # 3 & 1 and 2 & 2 both meet
    ((2, 3, 0), (1, 1, 0), False),                  # 3 & 1 meets, 1 & 2 does not
    ((4, 1, 0), (1, 4, 0), True),                   # each mask meets the other's category
    ((4, 1, 0), (1, 2, 0), False),                  # one side's mask misses
    ((0x80000000, ALL, 0), (1, 0x80000000, 0), True),      # the top bit
]


@pytest.mark.parametrize("a,b,want", TRUTH)
def test_truth_table(a, b, want):
    fa, fb = _f(*a), _f(*b)
    assert bool(spec.should_collide(fa, fb)) == want
    assert bool(spec.should_collide(fb, fa)) == want                 # the rule is symmetric


def test_rule_vectorised_matches_scalar():
    rng = np.random.default_rng(3)
    n = 500
    f = spec.filters(n, rng.integers(0, 8, n), rng.integers(0, 8, n), rng.integers(-2, 3, n))
    a, b = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    v = spec.pair_passes(f, a, b)
    for k in range(0, 2000, 37):
        fa, fb = f[a[k]], f[b[k]]
        if fa["group"] == fb["group"] and fa["group"] != 0:
            want = fa["group"] > 0
        else:
            want = (fa["mask"] & fb["category"]) != 0 and (fb["mask"] & fa["category"]) != 0
        assert v[k] == want


def _records(n):
    b = np.zeros(n, dtype=rigid_body_dtype)
    b["index"] = np.arange(n, dtype=np.uint32)
    b["pos"]["x"] = np.arange(n, dtype=np.float32) * 10.0
    b["velocity"]["y"] = -np.arange(n, dtype=np.float32)
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
    """Five bodies; body 2 becomes a ghost (mask 0): manifolds (0,1) x2 points, (1,2) x1, (0,3) x1, (2,4) dead; joints on slots 0, 2, 1, 6.
    (1,2) and (2,4) go; (0,1) and (0,3) stay at 0 and 1; joints 0, 2 (slots 0, 1) and 3 (slot 6 -> 2) stay; joint 1 (slot 2) goes."""
    st = _state(_records(5), [(0, 1, 2), (1, 2, 1), (0, 3, 1), (2, 4, 0)], np.array([0, 2, 1, -1, 3, 7, 9, -1], dtype=np.int32), [0, 2, 1, 4])
    st[3]["contact_point_index"][3] = 4
    f = spec.filters(5)
    f["mask"][2] = 0
    (b, m, c, j), dropped = spec.drop(st, f)
    assert dropped == 2
    assert b.tobytes() == st[0].tobytes()                               # bodies unchanged
    assert [tuple(x) for x in m] == [(0, 1, 2, 0), (0, 3, 1, 2)]
    assert c["solver_index"].tolist() == [0, 1, 2, 7]                 # live slots follow their joints; the dead slot stays byte for byte
    assert c["normal"]["y"].tolist() == [0.0, 1.0, 4.0, 5.0]
    assert j["contact_point_index"].tolist() == [0, 1, 2]
    assert j["normal_acc"].tolist() == [1.0, 3.0, 4.0]
    assert removal_spec.set_state_problems((b, m, c, j)) == []


def test_worked_example_nothing_and_everything():
    st = _state(_records(4), [(0, 1, 1), (2, 3, 2)], np.array([0, -1, 1, 2], dtype=np.int32), [0, 2, 3])
    (b, m, c, j), dropped = spec.drop(st, spec.filters(4))
    assert dropped == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip((b, m, c, j), st))
    (b, m, c, j), dropped = spec.drop(st, spec.filters(4, group=-1))
    assert dropped == 2 and len(m) == len(c) == len(j) == 0 and len(b) == 4
    f = spec.filters(4, category=[1, 1, 2, 2], mask=[1, 1, 2, 2])     # two layers: (0,1) and (2,3) stay
    assert spec.drop(st, f)[1] == 0
    f["mask"][3] = 1
    (b, m, c, j), dropped = spec.drop(st, f)
    assert dropped == 1 and m.tolist() == [(0, 1, 1, 0)] and j["contact_point_index"].tolist() == [0]


def _random_state(rng, nb):
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
    f = spec.filters(nb, rng.integers(0, 4, nb), rng.integers(0, 4, nb), rng.integers(-1, 2, nb))
    (b, m, c, j), dropped = spec.drop(st, f)
    assert removal_spec.set_state_problems((b, m, c, j)) == []
    keep = spec.pair_passes(f, st[1]["body1"], st[1]["body2"])
    assert dropped == int((~keep).sum()) and len(m) == int(keep.sum())
    assert spec.pair_passes(f, m["body1"], m["body2"]).all()            # no kept manifold holds a failing pair
    assert (m[["body1", "body2", "point_count"]] == st[1][keep][["body1", "body2", "point_count"]]).all()
    assert len(j) == int(m["point_count"].sum())                         # a joint per live slot of the kept manifolds
    assert (j["normal_acc"] == st[3]["normal_acc"][keep[st[3]["contact_point_index"] // 2]]).all()
    # dropping twice drops nothing more
    assert spec.drop((b, m, c, j), f)[1] == 0


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    idx = np.zeros(1, dtype=np.int32)
    f = spec.filters(1)
    out = np.zeros(1, dtype=collision_filter_dtype)
    dropped = C.c_int32(7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_set_collision_filters(None, vp(idx), vp(f), 1, C.byref(dropped)) == -1
    assert L.phx_world_get_collision_filters(None, vp(out), 1) == -1
    assert b"null handle" in L.phx_last_error()


def test_struct_size(tmp_path, built_lib):
    assert collision_filter_dtype.itemsize == 12
    assert [collision_filter_dtype.fields[k][1] for k in ("category", "mask", "group")] == [0, 4, 8]
    src = tmp_path / "size.c"
    src.write_text('#include "phyx_amd.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(phx_collision_filter) == 12, \"size\");\n"
                   "_Static_assert(offsetof(phx_collision_filter, group) == 8, \"group\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")])


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world():
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = _NoC(), None
    return w


@pytest.mark.parametrize("bodies", [np.zeros((2, 2), dtype=np.int32), np.array([0.0, 1.0]), np.zeros(3, dtype=bool), np.array([2 ** 40]), [["a"]]])
def test_set_refuses_bad_indices(bodies):
    with pytest.raises((TypeError, ValueError)):
        _world().set_collision_filters(bodies, 1, ALL, 0)


@pytest.mark.parametrize("kw", [dict(category=1.0), dict(mask=True), dict(group="x"), dict(category=-1), dict(category=2 ** 32),
                                dict(mask=2 ** 32), dict(group=2 ** 31), dict(group=-2 ** 31 - 1), dict(category=[1, 2, 3]),
                                dict(mask=np.ones((2, 1), dtype=np.uint32)), dict(group=np.array([0.5, 1.0]))])
def test_set_refuses_bad_values(kw):
    with pytest.raises((TypeError, ValueError)):
        _world().set_collision_filters(np.array([0, 1], dtype=np.int32), **kw)
