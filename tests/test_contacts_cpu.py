"""Contact reports (include/phyx_amd.h, CONTACTS) without a GPU: the entry points refuse a null handle, the Python wrappers refuse bad
input before any C call and retry a too-small buffer once, the specification (tests/contact_spec.py) agrees with itself on hand-built
states and on states stepped by the CPU oracle world, and examples/contacts.c builds and fails loudly without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_spec as spec
from phyx_amd.api import contact_dtype, contact_joint_dtype, contact_marker_dtype, contact_point_dtype, manifold_dtype, rigid_body_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    b = np.zeros(4, dtype=np.int32)
    off = np.zeros(8, dtype=np.int32)
    out = np.zeros(4, dtype=contact_dtype)
    t1, t2 = C.c_int64(0), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_query_contacts(None, vp(b), 1, 0, vp(off), vp(out), 4, C.byref(t1)) == -1
    assert L.phx_world_contact_events(None, vp(off), 2, C.byref(t1), vp(off), 2, C.byref(t2)) == -1
    assert L.phx_world_get_contact_markers_device(None, None, 0) == -1
    assert L.phx_world_contact_index(None, None) == -1
    assert b"null handle" in L.phx_last_error()


def test_struct_sizes():
    assert contact_dtype.itemsize == 40 and contact_marker_dtype.itemsize == 24
    assert contact_dtype.fields["point"][1] == 16 and contact_dtype.fields["normal_impulse"][1] == 32
    assert contact_marker_dtype.fields["live"][1] == 16


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world(lib=None):
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = lib if lib is not None else _NoC(), None
    return w


@pytest.mark.parametrize("bodies", [np.zeros((2, 2), dtype=np.int32), np.array([0.0, 1.0]), np.array([-1], dtype=np.int32),
                                    np.array([2 ** 40]), np.zeros(3, dtype=bool), [["a"]]])
def test_contacts_refuses_bad_input(bodies):
    with pytest.raises((TypeError, ValueError)):
        _world().contacts(bodies)


@pytest.mark.parametrize("out,cap", [("x", None), (None, None), (1.5, None), (True, None), (4096, -1), (4096, 2 ** 31), (4096, 1.0)])
def test_markers_refuse_bad_input(out, cap):
    with pytest.raises((TypeError, ValueError)):
        _world().contact_markers_device(out, cap)


class _Recorder:
    """Answers phx_world_query_contacts / phx_world_contact_events with PHX_ERR_CAPACITY while the caps are short."""

    def __init__(self, counts, nbegin=0, nend=0):
        self.counts, self.caps, self.flags, self.ev_caps = counts, [], [], []
        self.nbegin, self.nend = nbegin, nend

    def phx_world_counts(self, h, nb, nm, ncp, nj):
        for p, v in ((nb, 10), (nm, 3), (ncp, 6), (nj, 0)):
            C.cast(p, C.POINTER(C.c_int32))[0] = v
        return 0

    def phx_world_query_contacts(self, h, bodies, count, flags, offsets, out, cap, total):
        self.caps.append(cap); self.flags.append(flags)
        off = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_int32)), shape=(count + 1,))
        off[:] = np.concatenate([[0], np.cumsum(self.counts)])
        n = int(off[-1])
        C.cast(total, C.POINTER(C.c_int64))[0] = n
        if n > cap:
            return -4
        rec = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(cap * 40,)).view(contact_dtype)
        rec["other"][:n] = np.arange(n)
        return 0

    def phx_world_contact_events(self, h, begin, bcap, btotal, end, ecap, etotal):
        self.ev_caps.append((bcap, ecap))
        C.cast(btotal, C.POINTER(C.c_int64))[0] = self.nbegin
        C.cast(etotal, C.POINTER(C.c_int64))[0] = self.nend
        if self.nbegin > bcap or self.nend > ecap:
            return -4
        b = np.ctypeslib.as_array(C.cast(begin, C.POINTER(C.c_int32)), shape=(2 * bcap,))
        b[:2 * self.nbegin] = np.arange(2 * self.nbegin)
        e = np.ctypeslib.as_array(C.cast(end, C.POINTER(C.c_int32)), shape=(2 * ecap,))
        e[:2 * self.nend] = -np.arange(2 * self.nend)
        return 0


def test_contacts_retry_once_with_the_reported_size():
    r = _Recorder([300, 0, 700])
    off, rec = _world(r).contacts([1, 2, 3], skip_static=True)
    assert r.caps == [256, 1000] and r.flags == [1, 1]
    assert off.tolist() == [0, 300, 300, 1000] and len(rec) == 1000 and rec["other"].tolist() == list(range(1000))


def test_events_retry_once_with_the_reported_sizes():
    r = _Recorder([], nbegin=10, nend=100)
    begin, end = _world(r).contact_events()
    assert r.ev_caps == [(64, 64), (64, 100)]
    assert begin.shape == (10, 2) and end.shape == (100, 2) and begin.dtype == np.int32
    assert begin.ravel().tolist() == list(range(20)) and end.ravel().tolist() == [-k for k in range(200)]


# ---- the specification on hand-built states -------------------------------------------------------------------------------------------
def _state(rng, n=12, nm=20, static=(0,)):
    """Random bodies, manifolds between random distinct pairs (one duplicate pair), random live counts, joints for most live slots."""
    b = np.zeros(n, dtype=rigid_body_dtype)
    b["pos"]["x"] = rng.uniform(-100, 100, n).astype(F)
    b["pos"]["y"] = rng.uniform(-100, 100, n).astype(F)
    b["inv_mass"] = 1.0
    b["inv_inertia"] = 1.0
    for s in static:
        b["inv_mass"][s] = 0.0
        b["inv_inertia"][s] = 0.0
    m = np.zeros(nm, dtype=manifold_dtype)
    for i in range(nm):
        a, c = sorted(rng.choice(n, 2, replace=False))
        m[i] = (a, c, rng.integers(0, 3), 2 * i)
    m[nm - 1]["body1"], m[nm - 1]["body2"] = m[0]["body1"], m[0]["body2"]      # (set_state does not forbid a duplicate pair)
    m[1]["point_count"] = 2
    cps = np.zeros(2 * nm, dtype=contact_point_dtype)
    for f in ("delta1", "delta2", "normal"):
        cps[f]["x"] = rng.uniform(-5, 5, 2 * nm).astype(F)
        cps[f]["y"] = rng.uniform(-5, 5, 2 * nm).astype(F)
    cps["normal"]["x"][3] = 0.0                                         # (negation gives -0.0)
    cps["is_newly_created"] = rng.integers(0, 2, 2 * nm)
    cps["solver_index"] = -1
    live = [(i, k) for i in range(nm) for k in range(m[i]["point_count"])]
    j = np.zeros(len(live), dtype=contact_joint_dtype)
    for q, (i, k) in enumerate(live):
        cps["solver_index"][2 * i + k] = q
        j[q] = (2 * i + k, m[i]["body1"], m[i]["body2"], rng.uniform(0, 50), rng.uniform(-9, 9))
    cps["solver_index"][2 * live[0][0] + live[0][1]] = len(j) + 5     # out of range: no joint
    if len(live) > 1:
        cps["solver_index"][2 * live[1][0] + live[1][1]] = -1
    return b, m, cps, j


@pytest.mark.parametrize("seed", range(6))
def test_spec_is_symmetric(seed):
    """b lists a iff a lists b, record for record: the same manifold and slot, negated normals, equal impulses and flags."""
    b, m, cps, j = _state(np.random.default_rng(seed))
    n = len(b)
    off, rec = spec.contacts(b, m, cps, j, np.arange(n))
    assert off[-1] == 2 * int(np.clip(m["point_count"], 0, 2).sum())
    for x in range(n):
        for r in rec[off[x]:off[x + 1]]:
            y = r["other"]
            mine = rec[off[y]:off[y + 1]]
            back = mine[(mine["manifold"] == r["manifold"]) & (mine["slot"] == r["slot"])]
            assert len(back) == 1 and back[0]["other"] == x
            assert back[0]["normal"].tobytes() == (-r["normal"]).tobytes()
            assert back[0]["normal_impulse"] == r["normal_impulse"] and back[0]["friction_impulse"] == r["friction_impulse"]
            assert back[0]["flags"] == r["flags"]
            mm = m[r["manifold"]]
            cp = cps[mm["point_index"] + r["slot"]]
            d = cp["delta1"] if mm["body1"] == x else cp["delta2"]
            assert r["point"][0] == F(b["pos"]["x"][x]) + F(d["x"]) and r["point"][1] == F(b["pos"]["y"][x]) + F(d["y"])
        keys = [(r["other"], r["manifold"], r["slot"]) for r in rec[off[x]:off[x + 1]]]
        assert keys == sorted(keys)


def test_spec_dead_slots_no_joint_and_skip_static():
    b, m, cps, j = _state(np.random.default_rng(11))
    n = len(b)
    off, rec = spec.contacts(b, m, cps, j, np.arange(n))
    assert set(rec["slot"].tolist()) <= {0, 1}
    for r in rec:
        assert r["slot"] < m[r["manifold"]]["point_count"]             # dead slots give nothing
    si = cps["solver_index"][m["point_index"][rec["manifold"]] + rec["slot"]]
    nojoint = (si < 0) | (si >= len(j))
    assert nojoint.any()
    assert ((rec["flags"] & 2) != 0).tolist() == nojoint.tolist()
    assert (rec["normal_impulse"][nojoint] == 0).all() and (rec["friction_impulse"][nojoint] == 0).all()
    assert ((rec["flags"] & 1) != 0).tolist() == (cps["is_newly_created"][m["point_index"][rec["manifold"]] + rec["slot"]] != 0).tolist()
    so, sr = spec.contacts(b, m, cps, j, np.arange(n), skip_static=True)
    assert not (sr["other"] == 0).any()
    assert len(sr) == len(rec) - int((rec["other"] == 0).sum())
    # repeats: each listing has its own segment
    o2, r2 = spec.contacts(b, m, cps, j, [3, 3, 0, 3])
    seg = lambda o, r, q: r[o[q]:o[q + 1]].tobytes()      # noqa: E731
    assert seg(o2, r2, 0) == seg(o2, r2, 1) == seg(o2, r2, 3) == seg(off, rec, 3)
    assert seg(o2, r2, 2) == seg(off, rec, 0)
    e0, e1 = spec.contacts(b, m, cps, j, [])
    assert e0.tolist() == [0] and len(e1) == 0


def test_spec_events_compose():
    """B ∪ begin \\ end == T, begin ∩ B = ∅, end ⊆ B; the touching set drops duplicates and dead manifolds; the remap drops removed bodies."""
    rng = np.random.default_rng(3)
    prev = np.zeros((0, 2), dtype=np.int32)
    for s in range(8):
        b, m, cps, j = _state(rng)
        t = spec.touching(m)
        assert len(t) == len({(int(x), int(y)) for x, y in zip(m["body1"][m["point_count"] > 0], m["body2"][m["point_count"] > 0])})
        assert [tuple(p) for p in t] == sorted(tuple(p) for p in t)
        begin, end = spec.diff(t, prev)
        got = ({tuple(p) for p in prev} | {tuple(p) for p in begin}) - {tuple(p) for p in end}
        assert got == {tuple(p) for p in t}
        assert not ({tuple(p) for p in begin} & {tuple(p) for p in prev}) and {tuple(p) for p in end} <= {tuple(p) for p in prev}
        prev = t
    new = np.arange(12, dtype=np.int32)
    new[[2, 7]] = -1
    new[new >= 0] = np.arange(10)
    r = spec.remap(prev, new)
    assert len(r) == int((~np.isin(prev, [2, 7]).any(axis=1)).sum())
    assert [tuple(p) for p in r] == sorted(tuple(p) for p in r)


def test_spec_markers():
    b, m, cps, j = _state(np.random.default_rng(5))
    mk = spec.markers(b, m, cps)
    assert len(mk) == 2 * len(m)
    for i in range(len(mk)):
        mm = m[i // 2]
        if i - mm["point_index"] < mm["point_count"]:
            assert mk[i]["live"] == 1 and mk[i]["newly_created"] == cps[i]["is_newly_created"]
            assert mk[i]["point1"][0] == F(b["pos"]["x"][mm["body1"]]) + F(cps[i]["delta1"]["x"])
            assert mk[i]["point2"][1] == F(b["pos"]["y"][mm["body2"]]) + F(cps[i]["delta2"]["y"])
        else:
            assert mk[i].tobytes() == bytes(24)


def test_spec_on_oracle_worlds(oracle):
    """The oracle world (World::Update on the CPU) stepped 40 times: the spec's contacts and events stay consistent with its manifolds."""
    from phyx_amd import scenes
    w = oracle.OracleWorld(gravity=-200.0)
    w.add_scene(scenes.stack(4, 10))
    prev = np.zeros((0, 2), dtype=np.int32)
    as_ = lambda x, dt: np.frombuffer(x.tobytes(), dtype=dt)      # noqa: E731
    seen = 0
    for s in range(40):
        w.update(1.0 / 60.0, oracle.SOLVE_AVX2, oracle.ISLAND_MULTIPLE_SLOPPY)
        b, m = as_(w.bodies(), rigid_body_dtype), as_(w.manifolds(), manifold_dtype)
        cps, j = as_(w.contact_points(), contact_point_dtype), as_(w.joints(), contact_joint_dtype)
        n = len(b)
        off, rec = spec.contacts(b, m, cps, j, np.arange(n))
        assert off[-1] == 2 * int(np.clip(m["point_count"], 0, 2).sum())
        live = rec["flags"] & 2 == 0
        seen += int(live.sum())
        # a live joint's impulses are the record's
        si = cps["solver_index"][m["point_index"][rec["manifold"]] + rec["slot"]]
        assert (rec["normal_impulse"][live] == j["normal_acc"][si[live]]).all()
        t = spec.touching(m)
        begin, end = spec.diff(t, prev)
        assert ({tuple(p) for p in prev} | {tuple(p) for p in begin}) - {tuple(p) for p in end} == {tuple(p) for p in t}
        prev = t
    assert seen > 0 and len(prev) > 0


def test_contacts_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = str(tmp_path / "contacts")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "contacts.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        pytest.skip("a GPU is present: covered by the gpu test")
    r = subprocess.run([exe, "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
