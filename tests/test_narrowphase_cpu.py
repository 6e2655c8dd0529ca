"""The narrowphase corpus on the CPU (tests/narrowphase_corpus.py): which arms of the oracle's narrowphase it reaches
(the census), the traced per-pair entry against the oracle world's own result, and the oracle world against the reference's own
World / Collider through every phase."""
import numpy as np
import pytest

from oracle import binding as ob
import narrowphase_corpus as nc
import reference_runs as rr
from helpers import oracle_set_pose, oracle_set_velocity

DT = 1.0 / 60.0
MODE = (ob.SOLVE_AVX2, ob.ISLAND_SINGLE, 4, 4)


def _pose_all(world_set_pose, world_set_velocity, frames):
    for i, f in enumerate(frames):
        world_set_pose(i, f)
        world_set_velocity(i, (0.0, 0.0, 0.0))


def _bit(masks, i):
    return (masks[:, i >> 6] >> np.uint64(i & 63) & np.uint64(1)).astype(bool)


@pytest.fixture(scope="module")
def walk():
    """The oracle world through all phases with the trace on.  Per phase: the state before the step (bodies as posed, manifolds,
    contact points), the trace records, the new-pair count, and the state after."""
    cs = nc.cases()
    ow = ob.OracleWorld(0.0)
    ow.add_scene(nc.scene(cs))
    ow.set_trace(True)
    phases = []
    for p in range(nc.MAX_PHASES):
        frames = nc.phase_frames(cs, p)
        if p:
            _pose_all(lambda i, f: oracle_set_pose(ob, ow, i, f), lambda i, v: oracle_set_velocity(ow, i, v), frames)
        b = ow.bodies()
        placed = np.stack([b["pos"]["x"], b["pos"]["y"], b["xv"]["x"], b["xv"]["y"], b["yv"]["x"], b["yv"]["y"]], axis=1)
        assert placed.tobytes() == frames.tobytes(), "phase %d: the bodies are not at the corpus's frames" % p
        before = (b.copy(), ow.manifolds().copy(), ow.contact_points().copy())
        ow.update(DT, *MODE)
        phases.append({"before": before, "records": ow.trace_records(), "new": len(ow.new_pairs()), "summary": ow.trace_summary(),
                       "after": (ow.bodies().copy(), ow.manifolds().copy(), ow.contact_points().copy(), ow.joints().copy())})
    return {"cases": cs, "phases": phases, "overflows": ow.L.phxo_world_point_overflows(ow.h)}


def test_corpus_shape():
    cs = nc.cases()
    assert 2000 <= len(cs) <= 8000
    names = ob.trace_labels()
    assert sorted(nc.REQUIRED + list(nc.NOT_REQUIRED)) == sorted(names), "REQUIRED and NOT_REQUIRED together are the trace's labels, each once"
    for k, c in enumerate(cs):
        centre = np.array([(k % nc.GRID) * nc.PITCH, (k // nc.GRID) * nc.PITCH])
        assert 1 <= len(c.frames) <= nc.MAX_PHASES and c.size.max() <= 12 and c.size.min() >= 0
        reach = np.abs(c.frames[:, :, :2] - centre).max() + float(np.hypot(*c.size.max(axis=0)))
        assert reach < nc.PITCH / 2 - 1, "case %d leaves its cell" % k                     # so no box of one case nears another's
        assert c.frames.dtype == np.float32 and np.isfinite(c.frames).all()
        assert c.frames[0].tobytes() == np.stack([nc.frame(*c.start[0]), nc.frame(*c.start[1])]).tobytes()


def test_census(walk):
    cs, names = walk["cases"], ob.trace_labels()
    reached = {n: set() for n in names}
    big = False
    for p, ph in enumerate(walk["phases"]):
        rec = ph["records"]
        assert (rec["body1"] // 2 == rec["body2"] // 2).all(), "phase %d: a manifold joins two cases" % p
        labels, counts = ph["summary"]
        for i, n in enumerate(names):
            hit = _bit(rec["mask"], i)
            reached[n].update((rec["body1"][hit] // 2).tolist())
            assert counts.get(n, 0) == int(hit.sum()) and (n in labels) == bool(hit.any())      # the world's own accumulator
        alive = len(ph["before"][1])
        big = big or (alive >= 257 and alive % 256 != 0 and ph["new"] >= 100)
        for arr in ph["after"][:1] + ph["after"][2:]:
            for f in arr.dtype.names:
                if arr.dtype[f].kind == "f" or arr.dtype[f].names:
                    assert np.isfinite(np.frombuffer(np.ascontiguousarray(arr[f]).tobytes(), dtype=np.float32)).all(), (p, f)
    census = {n: len(s) for n, s in reached.items()}
    print("census:", census)
    short = {n: census[n] for n in nc.REQUIRED if census[n] < nc.MIN_CASES}
    assert not short, "REQUIRED labels reached by fewer than %d cases: %s" % (nc.MIN_CASES, short)
    assert not {n: census[n] for n in nc.NOT_REQUIRED if census[n]}, "a label held unreachable was reached"
    assert walk["overflows"] == 0
    assert big, "no phase with >= 257 live manifolds (not a multiple of 256) and >= 100 new pairs"


def test_traced_pair_entry_equals_the_world(walk):
    """Every manifold the oracle world updated, given to phxo_trace_pairs with its cached points: the same labels, the same point
    count and the same points as the world's own step left."""
    names = ob.trace_labels()
    dead_bit = names.index("dead")
    fields = ("delta1", "delta2", "normal", "is_merged", "is_newly_created")
    for p, ph in enumerate(walk["phases"]):
        bodies, m0, cp0 = ph["before"]
        rec = ph["records"]
        n = len(rec)
        old = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(m0["body1"], m0["body2"]))}
        pts = np.zeros(2 * n, dtype=ob.contact_point_dtype)
        pts["solver_index"] = -1
        cnt = np.zeros(n, dtype=np.int32)
        for k in range(n):
            i = old.get((int(rec["body1"][k]), int(rec["body2"][k])))
            if i is not None:
                cnt[k] = m0["point_count"][i]
                pts[2 * k:2 * k + 2] = cp0[m0["point_index"][i]:m0["point_index"][i] + 2]
        pair_bodies = bodies[np.stack([rec["body1"], rec["body2"]], axis=1).reshape(-1)]
        out, cnt_out, masks, over = ob.trace_pairs(pair_bodies, pts, cnt)
        assert over == 0
        assert masks.tobytes() == rec["mask"].tobytes(), "phase %d: labels differ" % p
        _, m1, cp1, _ = ph["after"]
        new = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(m1["body1"], m1["body2"]))}
        dead = _bit(masks, dead_bit)
        assert len(m1) == int((~dead).sum())
        for k in range(n):
            i = new.get((int(rec["body1"][k]), int(rec["body2"][k])))
            assert (i is None) == bool(dead[k])
            if i is None:
                assert cnt_out[k] == 0
                continue
            assert m1["point_count"][i] == cnt_out[k]
            for j in range(cnt_out[k]):
                a, b = cp1[m1["point_index"][i] + j], out[2 * k + j]
                assert all(a[f].tobytes() == b[f].tobytes() for f in fields), (p, k, j)


@pytest.mark.skipif(not ob.ref_full_can_pose("strict"), reason=ob.REF_POSE_SKIP)
def test_oracle_equals_the_reference_on_every_phase(walk):
    cs = walk["cases"]
    rw = ob.RefWorld("strict", 0.0, ob.PAIRS_PARALLEL)
    rw.add_scene(nc.scene(cs))
    contacts = 0
    for p, ph in enumerate(walk["phases"]):
        if p:
            _pose_all(rw.set_pose, rw.set_velocity, nc.phase_frames(cs, p))
        assert rw.bodies().tobytes() == ph["before"][0].tobytes(), "bodies differ before phase %d" % p
        rw.update(DT, *MODE)
        _, m, cp, j = ph["after"]
        assert rw.manifolds().tobytes() == m.tobytes(), "manifolds differ after phase %d" % p
        first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
        live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
        mine = cp[live].copy()
        mine["pad"] = 0
        assert rr.live_contact_points(rw).tobytes() == mine.tobytes(), "contact points differ after phase %d" % p
        rj = rw.joints()
        assert len(rj) == len(j)
        for f in ("contact_point_index", "body1", "body2"):
            assert (rj[f] == j[f]).all(), "joint %s differ after phase %d" % (f, p)
        contacts += len(rj)
    assert contacts > 0
