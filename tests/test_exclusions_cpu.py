"""Collision exclusions (include/phyx_amd.h, COLLISION EXCLUSIONS) without a GPU: the specification checks itself, agrees with
filter_spec.drop where the filters can say the same thing (all pairs among a set S == group -1 on S), keeps its order through a
removal's remap; the four entry points exist in the built library and in the binding and refuse a null handle; the Python wrapper
refuses bad input before any C call."""
import ctypes as C

import numpy as np
import pytest

import exclusion_spec as spec
import filter_spec
import removal_spec
from test_collision_filters_cpu import _NoC, _random_state, _records, _state

SYMBOLS = ("phx_world_add_collision_exclusions", "phx_world_remove_collision_exclusions", "phx_world_clear_collision_exclusions",
           "phx_world_get_collision_exclusions")


def test_normalize_sorts_and_orders():
    got = spec.normalize([(5, 2), (0, 9), (2, 5), (3, 1), (0, 4)])
    assert got.dtype == np.int32 and got.tolist() == [[0, 4], [0, 9], [1, 3], [2, 5]]
    assert spec.normalize([]).shape == (0, 2)
    with pytest.raises(AssertionError):
        spec.normalize([(1, 1)])


def test_membership_is_unordered():
    s = [(4, 1), (2, 3)]
    assert spec.excluded(s, [1, 4, 3, 1, 2, 0], [4, 1, 2, 3, 4, 0]).tolist() == [True, True, True, False, False, False]
    assert not spec.excluded([], [0, 1], [1, 0]).any()
    # a key is the pair, not a mix of its halves: (1, 2) is not (0, 2^32 + 2), nor (2, 1)'s neighbour (1, 3)
    assert spec.excluded([(1, 2)], [2, 1, 0], [1, 3, 2]).tolist() == [True, False, False]


def test_union_and_difference():
    s = spec.union([(1, 2), (3, 4)], [(4, 3), (0, 1)])
    assert s.tolist() == [[0, 1], [1, 2], [3, 4]]
    assert spec.union(s, s).tolist() == s.tolist()                        # a present pair changes nothing
    assert spec.difference(s, [(2, 1), (7, 8)]).tolist() == [[0, 1], [3, 4]]      # an absent pair is ignored
    assert spec.difference(s, s).shape == (0, 2)


def test_worked_example():
    """test_collision_filters_cpu's worked example with the pairs (1, 2) and (4, 2) excluded instead of body 2 ghosted: the same result."""
    st = _state(_records(5), [(0, 1, 2), (1, 2, 1), (0, 3, 1), (2, 4, 0)], np.array([0, 2, 1, -1, 3, 7, 9, -1], dtype=np.int32), [0, 2, 1, 4])
    st[3]["contact_point_index"][3] = 4
    (b, m, c, j), dropped = spec.drop(st, [(2, 1), (4, 2)])
    assert dropped == 2
    assert b.tobytes() == st[0].tobytes()
    assert [tuple(x) for x in m] == [(0, 1, 2, 0), (0, 3, 1, 2)]
    assert c["solver_index"].tolist() == [0, 1, 2, 7]
    assert j["contact_point_index"].tolist() == [0, 1, 2]
    assert j["normal_acc"].tolist() == [1.0, 3.0, 4.0]
    (b, m, c, j), dropped = spec.drop(st, [])
    assert dropped == 0 and all(x.tobytes() == y.tobytes() for x, y in zip((b, m, c, j), st))


@pytest.mark.parametrize("seed", range(8))
def test_drop_equals_the_filters_where_they_can_say_it(seed):
    """All pairs among a set S excluded == group -1 on S, byte for byte."""
    rng = np.random.default_rng(100 + seed)
    nb = int(rng.integers(4, 40))
    st = _random_state(rng, nb)
    S = np.flatnonzero(rng.integers(0, 2, nb)).tolist()
    pairs = [(a, b) for k, a in enumerate(S) for b in S[k + 1:]]
    f = filter_spec.filters(nb)
    f["group"][S] = -1
    want, want_dropped = filter_spec.drop(st, f)
    got, dropped = spec.drop(st, pairs)
    assert dropped == want_dropped
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert removal_spec.set_state_problems(got) == []
    assert not spec.excluded(pairs, got[1]["body1"], got[1]["body2"]).any()
    assert spec.drop(got, pairs)[1] == 0                                    # dropping twice drops nothing more


def test_remap_keeps_order():
    rng = np.random.default_rng(5)
    nb = 60
    pairs = spec.normalize([sorted(rng.choice(nb, size=2, replace=False).tolist()) for _ in range(150)])
    keep = rng.integers(0, 4, nb) > 0
    new = np.where(keep, np.cumsum(keep) - 1, -1)
    got = spec.remap(pairs, new)
    assert got.tolist() == spec.normalize(got).tolist(), "the remapped set is not sorted and normalized"
    assert len(got) == int((keep[pairs[:, 0]] & keep[pairs[:, 1]]).sum())
    old = np.flatnonzero(keep)
    assert old[got].tolist() == pairs[keep[pairs[:, 0]] & keep[pairs[:, 1]]].tolist()
    assert spec.remap(pairs, np.arange(nb)).tolist() == pairs.tolist()
    assert spec.remap(pairs, np.full(nb, -1)).shape == (0, 2)


def test_symbols_exist_in_library_and_binding(built_lib):
    from phyx_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.declared_symbols(), "%s has no prototype in phyx_amd/_lib.py" % name
        assert hasattr(built_lib, name), "libphyx_amd.so does not export %s" % name


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    p = np.array([[0, 1]], dtype=np.int32)
    n = C.c_int32(7)
    vp = p.ctypes.data_as(C.c_void_p)
    assert L.phx_world_add_collision_exclusions(None, vp, 1, C.byref(n)) == -1
    assert L.phx_world_remove_collision_exclusions(None, vp, 1) == -1
    assert L.phx_world_clear_collision_exclusions(None) == -1
    assert L.phx_world_get_collision_exclusions(None, vp, 1, C.byref(n)) == -1
    assert b"null handle" in L.phx_last_error()


def _world():
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = _NoC(), None
    return w


@pytest.mark.parametrize("pairs", [np.zeros(4, dtype=np.int32), np.zeros((2, 3), dtype=np.int32), np.array([[0.0, 1.0]]),
                                   np.array([[0, 2 ** 40]]), [["a", "b"]]])
def test_wrapper_refuses_bad_pairs(pairs):
    for call in ("add_collision_exclusions", "remove_collision_exclusions"):
        with pytest.raises((TypeError, ValueError)):
            getattr(_world(), call)(pairs)


def test_exclude_joined_refuses_unknown_kinds():
    with pytest.raises(ValueError):
        _world().exclude_joined(["hinge"])
    with pytest.raises(ValueError):
        _world().exclude_joined([7])
