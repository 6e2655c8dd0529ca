"""Contact reports on the device (include/phyx_amd.h, CONTACTS) held byte for byte to tests/contact_spec.py: contacts of all bodies and of
random listings on four scenes x four island modes x both paths after every step, and at the body counts where the index's and the events'
radix sorts change their digit split; touch events across steps and across removals, spawns,
set_state and refused calls; markers; no effect on the world; the index's caching; edges; the cfg 2 world; rejections; examples/contacts.c."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_spec as spec
import listing_cases
import phyx_amd
from phyx_amd import Configuration, DeviceBuffer, PhxError, scenes
from phyx_amd.api import contact_dtype, contact_marker_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0 / 60.0
G = -200.0
F = np.float32
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple": phyx_amd.ISLAND_MULTIPLE, "single_sloppy": phyx_amd.ISLAND_SINGLE_SLOPPY,
         "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
SCENES = {"stack": lambda: scenes.stack(6, 30),
          "wall": lambda: scenes.wall(14, 12),
          "falling": lambda: scenes.falling(300, width=80.0, ymax=260.0),
          "piles": lambda: scenes.piles(3, 50, ymax=220.0)}
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)


@pytest.fixture
def path(request, monkeypatch):
    """PHX_CONTACT_PATH for the worlds made in the test (read when a world is created)."""
    if request.param is None:
        monkeypatch.delenv("PHX_CONTACT_PATH", raising=False)
    else:
        monkeypatch.setenv("PHX_CONTACT_PATH", request.param)
    return request.param


def _world(scene, gravity=G):
    w = phyx_amd.World(0, gravity=gravity)
    w.add_scene(scene)
    return w


def _check_contacts(w, listed, skip, what, st=None):
    st = st if st is not None else w.state()
    off, rec = w.contacts(listed, skip_static=skip)
    so, sr = spec.contacts(*st, listed, skip)
    assert off.tobytes() == so.tobytes(), "offsets %s skip=%s" % (what, skip)
    assert rec.tobytes() == sr.tobytes(), "records %s skip=%s: first differing %s" % (
        what, skip, next((i for i in range(min(len(rec), len(sr))) if rec[i].tobytes() != sr[i].tobytes()), None))


def _events(w):
    begin, end = w.contact_events()
    assert begin.dtype == np.int32 and end.dtype == np.int32
    return begin, end


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_exact_on_scenes(built_lib, scene, mode, path):
    rng = np.random.default_rng(len(scene) * 7 + len(mode))
    w = _world(SCENES[scene]())
    cfg = Configuration(phyx_amd.SOLVE_AVX2, MODES[mode], 15, 15)
    n = w.counts()[0]
    prev = np.zeros((0, 2), dtype=np.int32)
    for s in range(30):
        w.Update(DT, cfg)
        st = w.state()
        every = np.arange(n, dtype=np.int32)
        some = rng.integers(0, n, size=int(rng.integers(1, 80))).astype(np.int32)
        for skip in (False, True):
            _check_contacts(w, every, skip, "%s/%s step %d all" % (scene, mode, s), st)
            _check_contacts(w, some, skip, "%s/%s step %d some" % (scene, mode, s), st)
        t = spec.touching(st[1])
        begin, end = _events(w)
        sb, se = spec.diff(t, prev)
        assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes(), "events step %d" % s
        prev = t
    assert len(prev) > 0


def _lonely_block_then(scene, n):
    """`scene` behind a block of isolated bodies that touch nothing, n bodies in all: the bodies that collide carry the highest indices."""
    lonely = n - len(scene["px"])
    assert lonely > 0
    i = np.arange(lonely)
    block = {"px": 1000.0 + 30.0 * (i % 64), "py": 500.0 + 30.0 * (i // 64), "angle": np.zeros(lonely), "sx": np.full(lonely, 5.0),
             "sy": np.full(lonely, 5.0), "static": np.zeros(lonely, dtype=bool)}
    return {k: np.concatenate([block[k], scene[k]]).astype(scene[k].dtype) for k in block}


@pytest.mark.parametrize("n", (255, 256, 257, 2047, 2048, 2049))
def test_body_counts_at_the_sort_key_splits(built_lib, monkeypatch, n):
    """The index sorts its entries, and the events their pairs, by body index with a radix sort whose digit split follows the key width (device_radix.h):
    key_bits(n - 1) and key_bits(n).  These body counts straddle 8 | 9 bits (one 8-bit pass | one 11-bit pass) and 11 | 12 bits (one 11-bit pass |
    two 8-bit passes, after which the result lies in the other buffer and the buffers' roles swap the other way)."""
    monkeypatch.setenv("PHX_CONTACT_PATH", "index")
    rng = np.random.default_rng(n)
    w = _world(_lonely_block_then(scenes.stack(3, 6), n))
    assert w.counts()[0] == n
    every = np.arange(n, dtype=np.int32)
    prev = np.zeros((0, 2), dtype=np.int32)
    for s in range(10):
        w.Update(DT, CFG)
        st = w.state()
        some = rng.integers(n - 25, n, size=40).astype(np.int32)
        for skip in (False, True):
            _check_contacts(w, every, skip, "n = %d step %d all" % (n, s), st)
            _check_contacts(w, some, skip, "n = %d step %d some" % (n, s), st)
        t = spec.touching(st[1])
        begin, end = _events(w)
        sb, se = spec.diff(t, prev)
        assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes(), "events n = %d step %d" % (n, s)
        prev = t
    m = w.manifolds
    assert len(prev) > 0 and len(m) > 0
    # only the scene at the end collides, and its last bodies do: the keys' upper digit has more than one non-empty bin wherever it can
    assert min(int(m["body1"].min()), int(m["body2"].min())) >= n - 19
    top = max(int(m["body1"].max()), int(m["body2"].max()))
    assert top == n - 1
    for edge in (256, 2048):
        if n > edge:
            assert top >= edge


def test_events_every_k_steps_and_the_first_call(built_lib):
    a, b = _world(scenes.piles(3, 50, ymax=220.0)), _world(scenes.piles(3, 50, ymax=220.0))
    for _ in range(5):
        a.Update(DT, CFG); b.Update(DT, CFG)
    t0 = spec.touching(a.manifolds)
    begin, end = _events(a)                                             # the first call: all of T begins
    assert begin.tobytes() == t0.tobytes() and len(end) == 0 and len(t0) > 0
    begin, end = _events(a)                                             # nothing happened since
    assert len(begin) == 0 and len(end) == 0
    prev = t0
    for k in (1, 3, 7, 2, 11):
        for _ in range(k):
            a.Update(DT, CFG); b.Update(DT, CFG)
        t = spec.touching(a.manifolds)
        begin, end = _events(a)
        sb, se = spec.diff(t, prev)
        assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes(), "k=%d" % k
        prev = t
    for x, y in zip(a.state(), b.state()):                              # (the events changed nothing else)
        assert x.tobytes() == y.tobytes()


def test_events_across_removal_and_spawn(built_lib):
    rng = np.random.default_rng(8)
    w = _world(scenes.piles(3, 50, ymax=220.0))
    for _ in range(20):
        w.Update(DT, CFG)
    _events(w)
    base = spec.touching(w.manifolds)
    # a removal remaps B through new[]: the next call diffs T against the remapped B
    gone = rng.choice(w.counts()[0], 30, replace=False)
    remap = w.remove_bodies(gone)
    base = spec.remap(base, remap)
    begin, end = _events(w)                                             # the removal made no pair start or stop
    assert len(begin) == 0 and len(end) == 0
    assert spec.touching(w.manifolds).tobytes() == base.tobytes()
    w.Update(DT, CFG)
    t = spec.touching(w.manifolds)
    begin, end = _events(w)
    sb, se = spec.diff(t, base)
    assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes()
    # a spawn leaves B alone (the new bodies touch nothing until a step)
    w.add_bodies(np.array([[x, 120.0, 0.2, 6.0, 4.0] for x in np.linspace(-150, 150, 20)], dtype=F))
    begin, end = _events(w)
    assert len(begin) == 0 and len(end) == 0
    for _ in range(3):
        w.Update(DT, CFG)
    t2 = spec.touching(w.manifolds)
    begin, end = _events(w)
    sb, se = spec.diff(t2, t)
    assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes()
    # removing every body empties B: the next call reports nothing, then the world is empty
    w.remove_bodies(np.arange(w.counts()[0]))
    assert [len(x) for x in _events(w)] == [0, 0]


def test_events_of_a_restored_twin(built_lib):
    """The original makes its events call, then is saved; a twin restored from that save reports the same events step for step."""
    a = _world(scenes.stack(6, 20))
    for _ in range(10):
        a.Update(DT, CFG)
    _events(a)
    st = a.state()
    b = phyx_amd.World(0, gravity=G)
    b.set_state(*st)
    assert [len(x) for x in _events(b)] == [0, 0]                       # (B := T(restored))
    b.set_state(*st)
    for s in range(15):
        if s == 7:
            a.set_velocities([5], [[300.0, 0.0, 0.0]]); b.set_velocities([5], [[300.0, 0.0, 0.0]])
        a.Update(DT, CFG); b.Update(DT, CFG)
        ea, eb = _events(a), _events(b)
        assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes(), "step %d" % s


def test_capacity_leaves_the_baseline(built_lib):
    w = _world(scenes.stack(6, 20))
    for _ in range(8):
        w.Update(DT, CFG)
    t = spec.touching(w.manifolds)
    assert len(t) > 2
    L = w.L
    beg = np.zeros((len(t), 2), dtype=np.int32)
    end = np.zeros((4, 2), dtype=np.int32)
    bt, et = C.c_int64(0), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_contact_events(w.h, vp(beg), len(t) - 1, C.byref(bt), vp(end), 4, C.byref(et)) == -4
    assert bt.value == len(t) and et.value == 0
    assert L.phx_world_contact_events(w.h, vp(beg), 0, C.byref(bt), vp(end), 0, C.byref(et)) == -4
    assert L.phx_world_contact_events(w.h, vp(beg), len(t), C.byref(bt), vp(end), 4, C.byref(et)) == 0
    assert beg.tobytes() == t.tobytes() and bt.value == len(t)
    # contacts: one short gives PHX_ERR_CAPACITY with the offsets and the total, then the exact result
    n = w.counts()[0]
    listed = np.arange(n, dtype=np.int32)
    so, sr = spec.contacts(*w.state(), listed)
    off = np.zeros(n + 1, dtype=np.int32)
    out = np.zeros(len(sr), dtype=contact_dtype)
    total = C.c_int64(0)
    assert L.phx_world_query_contacts(w.h, vp(listed), n, 0, vp(off), vp(out), len(sr) - 1, C.byref(total)) == -4
    assert total.value == len(sr) and off.tobytes() == so.tobytes()
    assert L.phx_world_query_contacts(w.h, vp(listed), n, 0, vp(off), vp(out), len(sr), C.byref(total)) == 0
    assert out.tobytes() == sr.tobytes()


def _every_body(w):
    listed = np.arange(w.counts()[0], dtype=np.int32)
    return (listed,) + spec.contacts(*w.state(), listed)


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_listing_protocol(built_lib, path):
    """phx_world_query_contacts with cap one short and exact (test_capacity_leaves_the_baseline's contacts half, on both paths), and a
    listed body that touches nothing in a world with manifolds."""
    w = listing_cases.world()
    listing_cases.one_short(w, "phx_world_query_contacts", "records", *_every_body(w))
    n, nm = w.counts()[:2]
    assert nm > 0
    w.add_bodies(np.array([[0.0, 5000.0, 0.0, 5.0, 5.0]], dtype=F))      # (far above the stack)
    listing_cases.counted_none(w, "phx_world_query_contacts", np.array([n, n], dtype=np.int32))


def test_scan_chunks_one_short(built_lib, monkeypatch):
    """cap one short on the chunked scan: 121 listed bodies in chunks of 7."""
    monkeypatch.setenv("PHX_CONTACT_PATH", "scan")
    monkeypatch.setenv("PHX_CONTACT_SCAN_CHUNK", "7")
    w = listing_cases.world()
    listing_cases.one_short(w, "phx_world_query_contacts", "records", *_every_body(w))


@pytest.mark.parametrize("scene", ("stack", "piles"))
def test_markers(built_lib, scene):
    w = _world(SCENES[scene]())
    assert w.counts()[1] == 0
    w.contact_markers_device(DeviceBuffer(24).address(), 0)            # (no manifold yet: nothing to write)
    for s in range(12):
        w.Update(DT, CFG)
        nm = w.counts()[1]
        buf = DeviceBuffer(24 * (2 * nm + 3))
        buf.from_host(np.full(24 * (2 * nm + 3), 0xAB, dtype=np.uint8))
        w.contact_markers_device(buf.address(), 2 * nm)
        w.sync()
        got = buf.to_host()
        b, m, cps, _ = w.state()
        want = spec.markers(b, m, cps)
        assert got[:48 * nm].tobytes() == want.tobytes(), "step %d" % s
        assert (got[48 * nm:] == 0xAB).all()                            # (nothing past 2 * nm)
    mk = want.view(contact_marker_dtype)
    assert (mk["live"] == 0).any() and (mk["live"] == 1).any()
    with pytest.raises(PhxError):
        w.contact_markers_device(buf.address(), 2 * nm - 1)
    with pytest.raises(PhxError):
        w.contact_markers_device(buf.address(4), 2 * nm)             # (8-byte alignment)


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_contacts_change_nothing(built_lib, path):
    """A world making all three calls between every step stays byte-equal to a twin that makes none, and keeps its cached schedule."""
    rng = np.random.default_rng(9)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
    a, b = _world(scenes.stack(6, 10), 0.0), _world(scenes.stack(6, 10), 0.0)
    a.contacts([0, 1])                                                  # (before the first step: host-staged bodies go up)
    n = a.counts()[0]
    buf = DeviceBuffer(24 * 4096)
    for s in range(20):
        a.contacts(rng.integers(0, n, 40)); a.contacts(np.arange(n), skip_static=True)
        a.contact_events()
        a.contact_markers_device(buf.address(), 4096)
        a.contact_index()
        a.Update(DT, cfg)
        b.Update(DT, cfg)
        assert a.solver.stats().recoloured == b.solver.stats().recoloured, "step %d" % s
    assert a.build_counts() == b.build_counts()
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.solver.stats().recoloured == 0


def test_index_is_cached_per_contact_epoch(built_lib, monkeypatch):
    monkeypatch.setenv("PHX_CONTACT_PATH", "index")
    w = _world(scenes.stack(6, 30))
    w.Update(DT, CFG)
    w.contacts([3, 4])
    b0 = w.contact_index()
    w.contacts(np.arange(100)); w.contacts([7], skip_static=True); w.contact_events()
    assert w.contact_index() == b0                                      # the same contact cache: no rebuild
    # set_poses moves a body but not the manifolds: no rebuild, yet the new pose shows in `point`
    before = w.contacts([20])[1]
    assert len(before)
    pose = w.body_states([20])[0]
    w.set_poses([20], [[pose["pos"]["x"] + 3.0, pose["pos"]["y"], pose["xv"]["x"], pose["xv"]["y"], pose["yv"]["x"], pose["yv"]["y"]]])
    off, after = w.contacts([20])
    assert w.contact_index() == b0
    assert (after["point"][:, 0] != before["point"][:, 0]).all()
    _check_contacts(w, np.array([20, 21, 20], dtype=np.int32), False, "after set_poses")
    w.set_velocities([4], [[1.0, 0.0, 0.0]]); w.add_accelerations([3], [[0.0, 10.0, 0.0]])
    assert w.contact_index() == b0
    w.Update(DT, CFG)
    assert w.contact_index() == b0 + 1
    w.add_bodies(np.array([[500.0, 50.0, 0.0, 5.0, 5.0]], dtype=F))     # (the body count changed: the offsets are sized by it)
    assert w.contact_index() == b0 + 2
    _check_contacts(w, np.arange(w.counts()[0], dtype=np.int32), True, "after add_bodies")
    w.remove_bodies([0])
    assert w.contact_index() == b0 + 3
    _check_contacts(w, np.arange(w.counts()[0], dtype=np.int32), False, "after remove_bodies")
    w.set_state(*w.state())
    assert w.contact_index() == b0 + 4


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_edges(built_lib, path, monkeypatch):
    rng = np.random.default_rng(12)
    # an empty world, and one before its first step
    e = phyx_amd.World(0, gravity=G)
    off, rec = e.contacts([])
    assert off.tolist() == [0] and len(rec) == 0
    assert [len(x) for x in _events(e)] == [0, 0]
    w = _world(scenes.piles(3, 50, ymax=220.0))
    off, rec = w.contacts([0, 1, 2])
    assert off.tolist() == [0, 0, 0, 0] and len(rec) == 0
    assert [len(x) for x in _events(w)] == [0, 0]
    for _ in range(10):
        w.Update(DT, CFG)
    st = w.state()
    n = w.counts()[0]
    for count in (0, 1, 63, 64, 65, 3000):
        listed = rng.integers(0, n, count).astype(np.int32)
        for skip in (False, True):
            _check_contacts(w, listed, skip, "count %d" % count, st)
    # a body with no contacts
    w.add_bodies(np.array([[5000.0, 500.0, 0.0, 3.0, 3.0]], dtype=F))
    w.Update(DT, CFG)
    off, rec = w.contacts([n, n, 0])
    assert off[1] == 0 and off[2] == 0
    _check_contacts(w, np.array([n, 0, n], dtype=np.int32), False, "lonely body")


@pytest.mark.parametrize("chunk", ("1", "7", "64"))
def test_scan_chunk_boundaries(built_lib, monkeypatch, chunk):
    monkeypatch.setenv("PHX_CONTACT_PATH", "scan")
    monkeypatch.setenv("PHX_CONTACT_SCAN_CHUNK", chunk)
    w = _world(scenes.piles(3, 50, ymax=220.0))
    for _ in range(10):
        w.Update(DT, CFG)
    n = w.counts()[0]
    listed = np.random.default_rng(int(chunk)).integers(0, n, 3 * int(chunk) + 5).astype(np.int32)
    listed[int(chunk) - 1:int(chunk) + 1] = 0                           # (the ground on both sides of the first boundary)
    for skip in (False, True):
        _check_contacts(w, listed, skip, "chunk %s" % chunk)


def test_cfg2_world(built_lib, monkeypatch):
    """The cfg 2 world (200 001 bodies) after 30 steps: contacts of every body and of 64 random bodies on both paths, and the events."""
    rng = np.random.default_rng(2)
    for p in ("scan", "index"):
        monkeypatch.setenv("PHX_CONTACT_PATH", p)
        w = _world(scenes.stack(1000, 200))
        for _ in range(30):
            w.Update(DT, CFG)
        st = w.state()
        n = len(st[0])
        _check_contacts(w, rng.integers(0, n, 64).astype(np.int32), False, "cfg 2 %s, 64 bodies" % p, st)
        _check_contacts(w, np.arange(n, dtype=np.int32), False, "cfg 2 %s, every body" % p, st)
        begin, end = _events(w)
        assert begin.tobytes() == spec.touching(st[1]).tobytes() and len(end) == 0
        w.Update(DT, CFG)
        t = spec.touching(w.manifolds)
        begin, end = _events(w)
        sb, se = spec.diff(t, spec.touching(st[1]))
        assert begin.tobytes() == sb.tobytes() and end.tobytes() == se.tobytes()
        del w


def test_rejections_leave_the_world_alone(built_lib, monkeypatch):
    a, b = _world(scenes.stack(6, 10)), _world(scenes.stack(6, 10))
    for _ in range(5):
        a.Update(DT, CFG); b.Update(DT, CFG)
    _events(a); _events(b)
    L = a.L
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    n = a.counts()[0]
    off = np.zeros(8, dtype=np.int32)
    out = np.zeros(64, dtype=contact_dtype)
    t1, t2 = C.c_int64(0), C.c_int64(0)
    for bad in ([-1], [n], [0, n + 5]):
        idx = np.array(bad, dtype=np.int32)
        assert L.phx_world_query_contacts(a.h, vp(idx), len(idx), 0, vp(off), vp(out), 64, C.byref(t1)) == -1
    idx = np.array([1], dtype=np.int32)
    assert L.phx_world_query_contacts(a.h, vp(idx), 1, 2, vp(off), vp(out), 64, C.byref(t1)) == -1      # flags
    assert L.phx_world_query_contacts(a.h, vp(idx), -1, 0, vp(off), vp(out), 64, C.byref(t1)) == -1     # count
    assert L.phx_world_query_contacts(a.h, vp(idx), 1, 0, vp(off), vp(out), -1, C.byref(t1)) == -1      # cap
    assert L.phx_world_query_contacts(a.h, None, 1, 0, vp(off), vp(out), 64, C.byref(t1)) == -1
    assert L.phx_world_query_contacts(a.h, vp(idx), 1, 0, None, vp(out), 64, C.byref(t1)) == -1
    assert L.phx_world_contact_events(a.h, vp(off), -1, C.byref(t1), vp(off), 2, C.byref(t2)) == -1
    assert L.phx_world_contact_events(a.h, None, 2, C.byref(t1), vp(off), 2, C.byref(t2)) == -1
    assert L.phx_world_contact_events(a.h, vp(off), 2, None, vp(off), 2, C.byref(t2)) == -1
    assert L.phx_world_get_contact_markers_device(a.h, None, -1) == -1
    # mid-step: PHX_ERR_STATE from all three
    a.PreSolve(DT); b.PreSolve(DT)
    assert L.phx_world_query_contacts(a.h, vp(idx), 1, 0, vp(off), vp(out), 64, C.byref(t1)) == -5
    assert L.phx_world_contact_events(a.h, vp(off), 4, C.byref(t1), vp(off), 4, C.byref(t2)) == -5
    buf = DeviceBuffer(24 * 4096)
    assert L.phx_world_get_contact_markers_device(a.h, buf.address(), 4096) == -5
    assert L.phx_world_contact_index(a.h, None) == -5
    a.FinishStep(DT, CFG); b.FinishStep(DT, CFG)
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    ea, eb = _events(a), _events(b)                                     # (B untouched by the refused calls)
    assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
    # a sharded world refuses the events call; its contacts answer from its own world
    a.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        a.contact_events()
    assert e.value.status == -5
    _check_contacts(a, np.arange(n, dtype=np.int32), False, "sharded")
    monkeypatch.setenv("PHX_CONTACT_PATH", "scna")
    with pytest.raises(PhxError, match="PHX_CONTACT_PATH"):
        phyx_amd.World(0)
    monkeypatch.setenv("PHX_CONTACT_PATH", "scan")
    monkeypatch.setenv("PHX_CONTACT_SCAN_CHUNK", "0")
    with pytest.raises(PhxError, match="PHX_CONTACT_SCAN_CHUNK"):
        phyx_amd.World(0)


def test_contacts_example_runs(tmp_path, built_lib):
    exe = str(tmp_path / "contacts")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "contacts.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe, "240"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "begin 1 - " in r.stdout or "begin 0 - 1" in r.stdout
    assert "body 1 touches" in r.stdout
