"""Collision exclusions (phx_world_add_collision_exclusions ...) on the device, held to tests/exclusion_spec.py, to the collision filters
where they can say the same thing, to an unfiltered twin world and to the oracle World:
  1. an active set that rejects nothing is the plain world (lockstep with the oracle);
  2. all pairs among a set S excluded == group -1 on S, byte for byte, the new-pair lists included;
  3. neighbours only — what the filters cannot say: per step the new pairs are an unfiltered twin's without the excluded ones, in order,
     the manifolds are the twin's, the solve is the oracle's;
  4. rows with more new pairs than the count pass remembers (the emit rescan);  5. a hub row (the chunk kernels);  6. both traits at once;
  7. remove / clear: an overlapping pair is new to the next step;  8. the set and its checks;  9. the other calls;  10. contact events;
  11. sleeping."""
import ctypes as C

import numpy as np
import pytest

import exclusion_spec as spec
import filter_spec
import phyx_amd
from helpers import oracle_world
from phyx_amd import Configuration, scenes
from phyx_amd.api import rigid_body_dtype
from spawn_lockstep import compare, step

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
ALL = 0xFFFFFFFF
NAMES = ("bodies", "manifolds", "contact points", "joints")
INVALID, CAPACITY, STATE = -1, -4, -5


def _cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def _world(scene, gravity=G):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    return pw


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _pairs(p):
    return np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1, 2))


def _live(manifolds):
    first, count = manifolds["point_index"].astype(np.int64), manifolds["point_count"].astype(np.int64)
    return np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)


def _same(a, b, what, live_points_only=False):
    assert a.counts() == b.counts(), "counts differ %s" % what
    live = _live(a.manifolds) if live_points_only else slice(None)
    for name, x, y in zip(NAMES, a.state(), b.state()):
        if name == "contact points":
            x, y = x[live], y[live]
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)


def _new_pairs(L, collider):
    n = C.c_int32(0)
    assert L.phx_broadphase_get_new_pairs(collider.h, None, 0, C.byref(n)) == 0
    out = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
    assert L.phx_broadphase_get_new_pairs(collider.h, _vp(out), len(out), C.byref(n)) == 0
    return out[:n.value]


def _row(count, pitch, y=15.0):
    """Ground (body 0) + `count` boxes of half-size 5x5 resting on it in one row, `pitch` apart: box i overlaps every box nearer than 10."""
    px = np.concatenate([[0.0], pitch * np.arange(count) - pitch * (count - 1) / 2.0])
    py = np.concatenate([[0.0], np.full(count, y)])
    sx = np.concatenate([[200.0], np.full(count, 5.0)])
    sy = np.concatenate([[10.0], np.full(count, 5.0)])
    return {"px": px.astype(np.float32), "py": py.astype(np.float32), "angle": np.zeros(count + 1, dtype=np.float32),
            "sx": sx.astype(np.float32), "sy": sy.astype(np.float32), "static": np.arange(count + 1) == 0}


def _neighbours(count):
    return _pairs([(i, i + 1) for i in range(1, count)])


def _twin_step(oracle, L, pf, passes, cfg, s):
    """One step of the world F against an unfiltered twin U = set_state(F's state) and the oracle's solver; `passes(body1, body2)`: the
    pairs F's settings let through.  Returns (the twin's new pairs, F's)."""
    pu = phyx_amd.World(0, gravity=G)
    pu.set_state(*pf.state())
    pf.PreSolve(DT)
    pu.PreSolve(DT)
    nf, nu = _new_pairs(L, pf.collider), _new_pairs(L, pu.collider)
    keep = passes(nu[:, 0], nu[:, 1]) if len(nu) else np.zeros(0, dtype=bool)
    assert nf.tobytes() == nu[keep].tobytes(), "step %d: the new pairs are not the twin's without the rejected ones, in order" % s
    mf, mu = pf.manifolds, pu.manifolds
    cf, cu = pf.contactPoints, pu.contactPoints
    assert passes(mf["body1"], mf["body2"]).all(), "step %d: a manifold holds a rejected pair" % s
    key = lambda m: (m["body1"].astype(np.uint64) << np.uint64(32)) | m["body2"].astype(np.uint64)      # noqa: E731
    ku = key(mu)
    order = np.argsort(ku, kind="stable")
    pos = np.searchsorted(ku[order], key(mf))
    assert (pos < len(ku)).all() and (ku[order][np.minimum(pos, len(ku) - 1)] == key(mf)).all(), "step %d: a manifold the twin lacks" % s
    k = order[pos]                                                          # the twin's manifold of each of F's
    assert len(mf) == int(passes(mu["body1"], mu["body2"]).sum()), "step %d: F's manifolds are not the twin's restricted to F's pairs" % s
    assert (mf["point_count"] == mu["point_count"][k]).all(), "step %d: point counts differ" % s
    cf, cu = cf.copy(), cu.copy()
    cf["solver_index"], cu["solver_index"] = 0, 0
    for q in range(2):
        live = mf["point_count"] > q
        i = np.flatnonzero(live)
        assert cf[2 * i + q].tobytes() == cu[2 * k[live] + q].tobytes(), "step %d: live slots %d differ" % (s, q)
    b, cp, j = pf.bodies, pf.contactPoints, pf.contactJoints
    pf.FinishStep(DT, cfg)
    order, offs = pf.solver.schedule()
    groups, _ = pf.solver.groups()
    ob, oj = b.view(oracle.body_dtype).copy(), j.view(oracle.joint_dtype).copy()
    oracle.solver_solve_grouped(ob, cp.view(oracle.contact_point_dtype), oj, order, offs, groups, cfg.contactIterationsCount,
                                cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    assert pf.contactJoints.tobytes() == oj.tobytes(), "step %d: impulses differ from the oracle's" % s
    got, want = pf.bodies, ob.view(rigid_body_dtype)
    assert got["velocity"].tobytes() == want["velocity"].tobytes(), "step %d: velocities differ" % s
    assert got["angular_velocity"].tobytes() == want["angular_velocity"].tobytes(), "step %d: angular velocities differ" % s
    return nu, nf


# ---- 1. an active set that rejects nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 5])
def test_active_set_that_rejects_nothing(oracle, built_lib, at):
    """stack(4, 12) with each box of column 0 paired with the box of column 3 in its row (they never overlap), added before the first
    step or after five, on the device: the excluded kernels run and nothing changes — bit-exact lockstep with the oracle for 40 steps.
    (The stack is still settling after five steps: the step behind the add rebuilds the schedule iff the plain world's does — measured,
    recoloured is 2 in both worlds on steps 4, 5 and 6; recoloured == 0 itself is asserted where a plain world reaches it:
    test_add_that_drops_nothing_keeps_the_schedule.)"""
    sc = scenes.stack(4, 12)
    cfg = _cfg()
    pw, ow, plain = _world(sc), oracle_world(sc), _world(sc)
    pairs = _pairs([(1 + r, 1 + 36 + r) for r in range(12)])
    for s in range(40):
        if s == at:
            assert pw.add_collision_exclusions(pairs) == 0
            assert pw.collision_exclusions().tolist() == spec.normalize(pairs).tolist()
        step(oracle, pw, ow, cfg, DT)
        plain.Update(DT, cfg)
        print("step %d: recoloured %d, the plain world %d" % (s, pw.solver.stats().recoloured, plain.solver.stats().recoloured))
        assert pw.solver.stats().recoloured == plain.solver.stats().recoloured, "step %d: the schedule was rebuilt where the plain world kept its own" % s
        compare(pw, ow, s)
    assert len(ow.joints()) > 0 and len(pw.collision_exclusions()) == 12


def test_add_that_drops_nothing_keeps_the_schedule(built_lib):
    """A stack at rest without gravity, once three steps in a row kept their schedule: an add on the device that drops nothing
    (dropped == 0) leaves the state as it is, and the next step has recoloured == 0."""
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pw = _world(scenes.stack(4, 12), gravity=0.0)
    seen = []
    for _ in range(60):
        pw.Update(DT, cfg)
        seen.append(pw.solver.stats().recoloured)
        if seen[-3:] == [0, 0, 0]:
            break
    assert seen[-3:] == [0, 0, 0], seen
    before = pw.state()
    assert pw.add_collision_exclusions(_pairs([(1 + r, 1 + 36 + r) for r in range(12)])) == 0
    for x, y in zip(before, pw.state()):
        assert x.tobytes() == y.tobytes()
    pw.Update(DT, cfg)
    assert pw.solver.stats().recoloured == 0, "an add that dropped nothing rebuilt the schedule"
    pw.remove_collision_exclusions(_pairs([(1, 37)]))                        # neither do a remove and a clear of pairs that do not overlap
    pw.Update(DT, cfg)
    assert pw.solver.stats().recoloured == 0
    pw.clear_collision_exclusions()
    pw.Update(DT, cfg)
    assert pw.solver.stats().recoloured == 0


# ---- 2. equal to the filters where the filters can say it ------------------------------------------------------------------------------
def test_equal_to_a_negative_group(built_lib):
    """World A: group -1 on S = column 1 of stack(4, 12); world B: all 66 pairs of S excluded; both after 5 steps, when manifolds among S
    exist.  Equal dropped counts, and byte-equal states and new-pair lists right after the call and after each of 40 further steps."""
    L, cfg = built_lib, _cfg()
    sc = scenes.stack(4, 12)
    pa, pb = _world(sc), _world(sc)
    for _ in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    S = np.arange(13, 25, dtype=np.int32)
    pairs = _pairs([(a, b) for k, a in enumerate(S) for b in S[k + 1:]])
    assert len(pairs) == 66
    before = pb.state()
    da = pa.set_collision_filters(S, group=-1)
    db = pb.add_collision_exclusions(pairs)
    assert da > 0 and db == da == spec.drop(before, pairs)[1]
    _same(pa, pb, "right after the call", live_points_only=True)
    for s in range(40):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        assert _new_pairs(L, pa.collider).tobytes() == _new_pairs(L, pb.collider).tobytes(), "new pairs differ at step %d" % s
        _same(pa, pb, "after step %d" % s, live_points_only=True)
        m = pb.manifolds
        assert not spec.excluded(pairs, m["body1"], m["body2"]).any()


def test_add_equals_set_state_of_drop(built_lib):
    """The add's compaction is set_state(exclusion_spec.drop(state)), byte for byte, dead slots included."""
    cfg = _cfg()
    pa = _world(scenes.stack(4, 12))
    for _ in range(8):
        pa.Update(DT, cfg)
    before = pa.state()
    pairs = _pairs([(0, 1), (14, 13), (15, 16), (30, 31), (2, 40)])
    want, want_dropped = spec.drop(before, pairs)
    assert want_dropped >= 4
    assert pa.add_collision_exclusions(pairs) == want_dropped
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*want)
    for name, x, y in zip(NAMES, pa.state(), pb.state()):
        assert x.tobytes() == y.tobytes(), "%s differ from set_state(drop(state))" % name
    assert pb.add_collision_exclusions(pairs) == 0
    for s in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)


# ---- 3. what the filters cannot say: neighbours only -----------------------------------------------------------------------------------
def test_neighbours_only(oracle, built_lib):
    """Ten boxes in a row 4 apart (box i overlaps i +- 1 and i +- 2) with {(i, i + 1)} excluded: the per-step twin check, 12 steps."""
    cfg = _cfg()
    pf = _world(_row(10, 4.0))
    pairs = _neighbours(10)
    assert pf.add_collision_exclusions(pairs) == 0
    passes = lambda a, b: ~spec.excluded(pairs, a, b)      # noqa: E731
    twin_excluded = twin_far = 0
    for s in range(12):
        nu, nf = _twin_step(oracle, built_lib, pf, passes, cfg, s)
        a, b = nu[:, 0].astype(np.int64), nu[:, 1].astype(np.int64)
        twin_excluded += int(spec.excluded(pairs, a, b).sum())
        twin_far += int(((a > 0) & (b > 0) & (np.abs(a - b) > 1)).sum())
    assert twin_excluded > 0, "the twin never emitted an excluded pair: the test's premise"
    assert twin_far > 0, "the twin never emitted a non-neighbour pair among the links: the test's premise"
    m = pf.manifolds
    assert ((m["body1"] > 0) & (m["body2"] > 0)).any() and pf.counts()[3] > 0


# ---- 4. ROW_CACHE overflow and the emit rescan -----------------------------------------------------------------------------------------
def test_rows_with_more_new_pairs_than_the_cache(oracle, built_lib):
    """clique(12): every row meets up to 11 new partners in step one, more than the count pass remembers (4), so the emit pass rescans
    them — with the count pass's test, or the offsets lie.  Every third pair among the boxes excluded."""
    sc = scenes.clique(12)
    boxes = [(a, b) for a in range(1, 13) for b in range(a + 1, 13)]
    pairs = _pairs(boxes[::3])
    pf = _world(sc)
    assert pf.add_collision_exclusions(pairs) == 0
    nu, nf = _twin_step(oracle, built_lib, pf, lambda a, b: ~spec.excluded(pairs, a, b), _cfg(), 0)
    assert np.unique(nu[:, 0], return_counts=True)[1].max() > 4, "no row of the twin found more than 4 new pairs: the test's premise"
    assert np.unique(nf[:, 0], return_counts=True)[1].max() > 4, "no row of F was rescanned: the test's premise"
    assert len(nf) < len(nu)


# ---- 5. hub row and the chunk kernels --------------------------------------------------------------------------------------------------
def test_hub_row(oracle, built_lib):
    """stack(210, 10): the ground's row has 2100 candidates, more than a row sweeps by itself (2048), so the chunk kernels sweep it.
    The ground is excluded with every 7th box of the bottom row."""
    sc = scenes.stack(210, 10)
    bottom = 1 + 10 * np.arange(0, 210, 7)
    pairs = _pairs([(0, int(b)) for b in bottom])
    pf = _world(sc)
    assert pf.add_collision_exclusions(pairs) == 0
    cfg = _cfg(phyx_amd.ISLAND_SINGLE_SLOPPY)
    missing = 0
    for s in range(3):
        nu, nf = _twin_step(oracle, built_lib, pf, lambda a, b: ~spec.excluded(pairs, a, b), cfg, s)
        ground = (nu[:, 0] == 0) | (nu[:, 1] == 0)
        missing += int(spec.excluded(pairs, nu[ground, 0], nu[ground, 1]).sum())
        assert len(nu) - len(nf) == int(spec.excluded(pairs, nu[:, 0], nu[:, 1]).sum())
    assert missing >= len(bottom), "the twin emitted no ground pair that F did not: the test's premise"
    m = pf.manifolds
    on_ground = np.concatenate([m["body2"][m["body1"] == 0], m["body1"][m["body2"] == 0]])
    assert len(on_ground) == 210 - len(bottom) and not np.isin(bottom, on_ground).any()


# ---- 6. both traits at once ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", ["every other box", "every other pair of boxes"])
def test_filters_and_exclusions_together(oracle, built_lib, layered):
    """Ten boxes in a row 3 apart (box i overlaps i +- 1, 2, 3), a filter layer {2, 2 | 4} on every other box (the ground is {4, ALL}) and the
    neighbour exclusions: the twin's pairs minus those failing either rule, in order.  Layered by pairs of boxes, some neighbours share
    a layer: pairs that only the exclusions reject."""
    cfg = _cfg()
    n = 11
    pf = _world(_row(10, 3.0))
    i = np.arange(n)
    on = (i % 2 == 0) if layered == "every other box" else ((i - 1) // 2 % 2 == 0)
    on &= i > 0
    filt = filter_spec.filters(n, np.where(i == 0, 4, np.where(on, 2, 1)), np.where(on, 2 | 4, ALL), 0)
    pf.set_collision_filters(i.astype(np.int32), filt["category"], filt["mask"], filt["group"])
    pairs = _neighbours(10)
    assert pf.add_collision_exclusions(pairs) == 0
    passes = lambda a, b: filter_spec.pair_passes(filt, a, b) & ~spec.excluded(pairs, a, b)      # noqa: E731
    only_filter = only_set = both = emitted = 0
    for s in range(8):
        nu, nf = _twin_step(oracle, built_lib, pf, passes, cfg, s)
        f, x = ~filter_spec.pair_passes(filt, nu[:, 0], nu[:, 1]), spec.excluded(pairs, nu[:, 0], nu[:, 1])
        only_filter += int((f & ~x).sum()); only_set += int((x & ~f).sum()); both += int((f & x).sum()); emitted += len(nf)
    assert only_filter > 0 and both > 0 and emitted > 0, (only_filter, only_set, both, emitted)
    if layered != "every other box":
        assert only_set > 0, "no pair was rejected by the exclusions alone: the test's premise"


# ---- 7. removal ------------------------------------------------------------------------------------------------------------------------
def test_remove_and_clear_make_overlapping_pairs_new(built_lib):
    L, cfg = built_lib, _cfg()
    pf = _world(_row(10, 4.0))
    pairs = _neighbours(10)
    pf.add_collision_exclusions(pairs)
    for _ in range(3):
        pf.Update(DT, cfg)
    x = pf.bodies["pos"]["x"]
    assert abs(float(x[4]) - float(x[3])) < 9.0, "boxes 3 and 4 no longer overlap: the test's premise"
    before = pf.state()
    pf.remove_collision_exclusions(_pairs([(4, 3)]))
    for a, b in zip(before, pf.state()):
        assert a.tobytes() == b.tobytes(), "remove touched the state"
    assert pf.collision_exclusions().tolist() == spec.difference(pairs, [(3, 4)]).tolist()

    def fresh(expected):
        nm_before = pf.counts()[1]
        pf.PreSolve(DT)
        new = _new_pairs(L, pf.collider).astype(np.int64)
        got = {(min(a, b), max(a, b)) for a, b in new.tolist()}
        assert expected <= got, "the pairs that may collide again are not among the new pairs"
        m, cp, j = pf.manifolds, pf.contactPoints, pf.contactJoints
        tail = m[len(m) - len(new):]
        assert len(m) == nm_before + len(new), "a manifold died in this step: the test's premise (nothing is packed)"
        assert np.stack([tail["body1"], tail["body2"]], axis=1).tolist() == new.tolist(), "the new manifolds are not the last ones"
        for q, (a, b) in enumerate(new.tolist()):
            if (min(a, b), max(a, b)) not in expected:
                continue
            mi = len(m) - len(new) + q
            assert tail["point_count"][q] > 0, "an overlapping pair got no contact points"
            for slot in range(int(tail["point_count"][q])):
                jt = j[cp["solver_index"][2 * mi + slot]]
                assert jt["contact_point_index"] == 2 * mi + slot and jt["normal_acc"] == 0.0 and jt["friction_acc"] == 0.0
        pf.FinishStep(DT, cfg)

    fresh({(3, 4)})
    rest = {tuple(p) for p in pf.collision_exclusions().tolist()}
    x = pf.bodies["pos"]["x"]
    still = {(a, b) for a, b in rest if abs(float(x[a]) - float(x[b])) < 9.0}
    assert len(still) >= 4
    pf.clear_collision_exclusions()
    assert pf.collision_exclusions().shape == (0, 2)
    fresh(still)
    pf.clear_collision_exclusions()                                        # empty already: a no-op
    pf.Update(DT, cfg)


# ---- 8. the set ------------------------------------------------------------------------------------------------------------------------
def test_the_set_and_its_checks(built_lib):
    L, cfg = built_lib, _cfg()
    pw = _world(scenes.stack(4, 12))
    n = pw.counts()[0]
    first = [(9, 2), (1, 3), (40, 0), (1, 2)]
    assert pw.add_collision_exclusions(_pairs(first)) == 0                  # before the first step: the set waits on the host
    want = spec.normalize(first)
    assert pw.collision_exclusions().tolist() == want.tolist() == [[0, 40], [1, 2], [1, 3], [2, 9]]
    for _ in range(6):
        pw.Update(DT, cfg)
    assert pw.add_collision_exclusions(_pairs([(2, 1), (3, 1)])) == 0       # present pairs: a no-op
    pw.remove_collision_exclusions(_pairs([(5, 6), (2, 3)]))                 # absent pairs: ignored
    pw.add_collision_exclusions(_pairs([]))
    pw.remove_collision_exclusions(_pairs([]))
    assert pw.collision_exclusions().tolist() == want.tolist()
    pw.add_collision_exclusions(_pairs([(30, 31), (2, 9)]))
    want = spec.union(want, [(30, 31)])
    pw.remove_collision_exclusions(_pairs([(3, 1), (7, 8)]))
    want = spec.difference(want, [(1, 3)])
    assert pw.collision_exclusions().tolist() == want.tolist()

    before = pw.state()
    count = C.c_int32(-7)
    dropped = C.c_int32(-7)

    def refused(call, p, cnt, code=INVALID, words=None):
        p = None if p is None else _pairs(p)
        args = (pw.h, None if p is None else _vp(p), cnt)
        st = L.phx_world_add_collision_exclusions(*args, C.byref(dropped)) if call == "add" else L.phx_world_remove_collision_exclusions(*args)
        assert st == code, (call, p, cnt, st)
        if words:
            assert words in L.phx_last_error(), L.phx_last_error()
        assert pw.collision_exclusions().tolist() == want.tolist()
        for a, b in zip(before, pw.state()):
            assert a.tobytes() == b.tobytes(), "a refused call changed the world"

    for call in ("add", "remove"):
        refused(call, [(1, 2)], -1, words=b"negative count")
        refused(call, None, 2, words=b"null array")
        refused(call, [(0, 1), (5, n)], 2, words=b"out of range")
        refused(call, [(-1, 4)], 1, words=b"out of range")
        refused(call, [(4, 5), (6, 6)], 2, words=b"twice")
        refused(call, [(4, 5), (7, 8), (5, 4)], 3, words=b"appears twice in one call")
        refused(call, [(4, 5), (4, 5)], 2, words=b"appears twice in one call")
    # get: always fills *count; a small cap is PHX_ERR_CAPACITY
    out = np.zeros((len(want), 2), dtype=np.int32)
    assert L.phx_world_get_collision_exclusions(pw.h, _vp(out), len(want) - 1, C.byref(count)) == CAPACITY and count.value == len(want)
    assert L.phx_world_get_collision_exclusions(pw.h, _vp(out), len(want), C.byref(count)) == 0 and out.tolist() == want.tolist()
    assert L.phx_world_get_collision_exclusions(pw.h, _vp(out), len(want), None) == 0
    # between pre_solve and finish_step: PHX_ERR_STATE
    twin = phyx_amd.World(0, gravity=G)
    twin.set_state(*before)
    twin.add_collision_exclusions(want)
    pw.PreSolve(DT)
    p = _pairs([(4, 5)])
    assert L.phx_world_add_collision_exclusions(pw.h, _vp(p), 1, None) == STATE
    assert L.phx_world_remove_collision_exclusions(pw.h, _vp(p), 1) == STATE
    assert L.phx_world_clear_collision_exclusions(pw.h) == STATE
    pw.FinishStep(DT, cfg)
    twin.Update(DT, cfg)
    _same(pw, twin, "after the refused calls and a step")
    assert pw.collision_exclusions().tolist() == want.tolist()


# ---- 9. the other calls ----------------------------------------------------------------------------------------------------------------
def test_removal_remaps_and_a_spawn_keeps_the_set(built_lib):
    cfg = _cfg()
    pw = _world(scenes.stack(4, 12))
    for _ in range(5):
        pw.Update(DT, cfg)
    rng = np.random.default_rng(9)
    n = pw.counts()[0]
    pairs = spec.normalize([sorted(rng.choice(n, size=2, replace=False).tolist()) for _ in range(60)])
    pw.add_collision_exclusions(pairs)
    remap = pw.remove_bodies(np.array([2, 9, 30, 31, 44], dtype=np.int32))
    want = spec.remap(pairs, remap)
    assert 0 < len(want) < len(pairs)
    assert pw.collision_exclusions().tolist() == want.tolist()
    pw.Update(DT, cfg)
    m = pw.manifolds
    assert not spec.excluded(want, m["body1"], m["body2"]).any()
    removed, everything = pw.remove_outside((-1e6, -1e6, 1e6, 1e6))          # every body inside: nothing changes
    assert removed == 0 and (everything == np.arange(len(everything))).all() and pw.collision_exclusions().tolist() == want.tolist()
    # a spawn leaves the set alone, and the new bodies collide: two boxes dropped onto each other above the pile
    rows = np.array([[45.0, 15.0, 0.0, 5.0, 5.0], [47.0, 18.0, 0.0, 5.0, 5.0]], dtype=np.float32)
    new = pw.add_bodies(rows)
    assert pw.collision_exclusions().tolist() == want.tolist()
    pw.Update(DT, cfg)
    m = pw.manifolds
    got = {(min(a, b), max(a, b)) for a, b in zip(m["body1"].tolist(), m["body2"].tolist())}
    assert (int(new[0]), int(new[1])) in got and (0, int(new[0])) in got
    assert not spec.excluded(want, m["body1"], m["body2"]).any()
    # ... and a new body can be excluded
    assert pw.add_collision_exclusions(_pairs([(new[1], new[0])])) == 1
    pw.Update(DT, cfg)
    m = pw.manifolds
    assert not spec.excluded([(new[0], new[1])], m["body1"], m["body2"]).any()


def test_set_state_empties_the_set(built_lib):
    cfg = _cfg()
    pa = _world(_row(10, 4.0))
    pa.add_collision_exclusions(_neighbours(10))
    for _ in range(3):
        pa.Update(DT, cfg)
    pb = phyx_amd.World(0, gravity=G)
    pb.add_scene(_row(4, 20.0))
    pb.add_collision_exclusions(_pairs([(1, 2)]))
    pb.set_state(*pa.state())
    assert pb.collision_exclusions().shape == (0, 2), "set_state did not empty the set"
    pb.add_collision_exclusions(_neighbours(10))
    for s in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)


def test_snapshots_carry_the_set(built_lib):
    L, cfg = built_lib, _cfg()
    pa = _world(_row(10, 4.0))
    pairs = _neighbours(10)
    pa.add_collision_exclusions(pairs)
    for _ in range(4):
        pa.Update(DT, cfg)
    snap = pa.save()
    pb = pa.fork()
    assert pb.collision_exclusions().tolist() == pairs.tolist()
    for s in range(20):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "fork, after step %d" % s)
    m = pb.manifolds
    assert len(m) > 10 and not spec.excluded(pairs, m["body1"], m["body2"]).any()
    # the blob is layout version 1 and holds no exclusions
    n = C.c_size_t(0)
    assert L.phx_snapshot_blob_bytes(snap.h, C.byref(n)) == STATE and b"collision exclusions" in L.phx_last_error()
    buf = C.create_string_buffer(1 << 20)
    assert L.phx_snapshot_export(snap.h, buf, len(buf)) == STATE
    # a load of the older snapshot brings its set back (and a world that had another set loses it)
    pb.clear_collision_exclusions()
    pb.add_collision_exclusions(_pairs([(1, 9)]))
    pb.load(snap)
    pa.load(snap)
    assert pb.collision_exclusions().tolist() == pairs.tolist()
    for s in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "load, after step %d" % s)
    pa.clear_collision_exclusions()
    again = pa.save()
    assert len(again.to_bytes()) > 128
    pb.load(again)
    assert pb.collision_exclusions().shape == (0, 2)


def test_sharded_worlds_refuse(built_lib):
    L = built_lib
    pw = _world(scenes.stack(2, 3))
    p = _pairs([(1, 2)])
    pw.set_shard(0, 2)
    assert L.phx_world_add_collision_exclusions(pw.h, _vp(p), 1, None) == STATE
    assert L.phx_world_remove_collision_exclusions(pw.h, _vp(p), 1) == STATE
    assert L.phx_world_clear_collision_exclusions(pw.h) == STATE
    pw.set_shard(0, 1)
    pw.add_collision_exclusions(p)
    assert L.phx_world_set_shard(pw.h, 0, 2) == STATE and b"collision exclusions" in L.phx_last_error()
    pw.clear_collision_exclusions()
    assert L.phx_world_set_shard(pw.h, 0, 2) == 0


# ---- 10. contact events ----------------------------------------------------------------------------------------------------------------
def test_excluded_pairs_end_in_the_events(built_lib):
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pw = _world(scenes.stack(6, 10))
    for _ in range(60):
        pw.Update(DT, cfg)
    pw.contact_events()
    m = pw.manifolds
    touching = {(int(a), int(b)) for a, b, pc in zip(m["body1"], m["body2"], m["point_count"]) if pc > 0}
    gone = [p for p in sorted(touching) if 7 in p]      # (the pair set is keyed by ordered pairs: (6, 7) and (7, 6) may both have a manifold)
    assert len(gone) >= 2
    pairs = spec.normalize(gone)
    assert pw.add_collision_exclusions(pairs) == int(spec.excluded(pairs, m["body1"], m["body2"]).sum()) >= len(gone)
    begin, end = pw.contact_events()
    assert len(begin) == 0
    assert sorted(map(tuple, end.tolist())) == gone


# ---- 11. sleeping ----------------------------------------------------------------------------------------------------------------------
def test_add_wakes_the_components_it_names(built_lib):
    """Two boxes piled on a shelf and a third far away, all asleep: an add that names one box of the pile and the far box wakes both
    components; a remove and a clear wake what they name as well."""
    cfg = _cfg()
    pw = phyx_amd.World(0, gravity=G)
    pw.AddBody((0.0, 0.0), 0.0, (400.0, 10.0), static=True)
    low, high, far = (pw.AddBody((-100.0, 15.0), 0.0, (5.0, 5.0)), pw.AddBody((-100.0, 25.0), 0.0, (5.0, 5.0)), pw.AddBody((200.0, 15.0), 0.0, (5.0, 5.0)))
    pw.set_sleeping(20.0, 5.0, 3 * DT)

    def sleep():
        for _ in range(200):
            pw.Update(DT, cfg)
            if pw.sleep_counts()[0] == 3:
                return
        raise AssertionError("the boxes never came to rest: the test's premise")

    sleep()
    pw.add_collision_exclusions(_pairs([(far, high)]))
    assert pw.sleep_counts()[0] == 0, "the add did not wake the pile and the far box"
    sleep()
    pw.remove_collision_exclusions(_pairs([(low, far)]))                    # (an absent pair: its bodies are named all the same)
    assert pw.sleep_counts()[0] == 0
    sleep()
    pw.clear_collision_exclusions()                                        # the set holds (high, far): both components wake
    assert pw.sleep_counts()[0] == 0
    sleep()
    pw.clear_collision_exclusions()                                        # an empty set: nobody is named
    assert pw.sleep_counts()[0] == 3
