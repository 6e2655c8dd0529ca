"""The two-pass listing protocol of phx_world_query_aabb, _boxes and _contacts (include/phyx_amd.h: offsets and *total are valid on
PHX_ERR_CAPACITY), checked through the C entry points on one small world: scenes.stack(6, 20) after 8 steps, 121 bodies, the smallest
in which the query index has two levels (fan-out 64) and every listing below has hits.  The three calls share their argument list:
(world, rows, count, flags, offsets, out, cap, total)."""
import ctypes as C

import numpy as np

import phyx_amd
from phyx_amd import Configuration, scenes

DT = 1.0 / 60.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def world():
    """Made under the caller's PHX_*_PATH / PHX_*_SCAN_CHUNK (read when a world is created)."""
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_scene(scenes.stack(6, 20))
    for _ in range(8):
        w.Update(DT, CFG)
    return w


def one_short(w, name, noun, rows, so, want):
    """cap = total - 1: PHX_ERR_CAPACITY, the message, and the spec's total and offsets all the same; cap = total: the spec's bytes."""
    fn, count, total = getattr(w.L, name), len(rows), int(so[-1])
    assert total >= 2 and len(want) == total                           # ("one short" is not "none")
    offsets, out, t = np.full(count + 1, -1, dtype=np.int32), np.zeros(total, dtype=want.dtype), C.c_int64(-1)
    assert fn(w.h, _vp(rows), count, 0, _vp(offsets), _vp(out), total - 1, C.byref(t)) == -4
    assert w.L.phx_last_error() == b"%s: %d %s, room for %d" % (name.encode(), total, noun.encode(), total - 1)
    assert t.value == total and offsets.tobytes() == so.tobytes()
    offsets[:], t.value = -1, -1
    assert fn(w.h, _vp(rows), count, 0, _vp(offsets), _vp(out), total, C.byref(t)) == 0
    assert t.value == total and offsets.tobytes() == so.tobytes() and out.tobytes() == want.tobytes()


def counted_none(w, name, rows):
    """Rows that list nothing in a world that has something to list: no output buffer is needed, every offset and the total are 0."""
    count = len(rows)
    assert count > 0
    offsets, t = np.full(count + 1, -1, dtype=np.int32), C.c_int64(-1)
    assert getattr(w.L, name)(w.h, _vp(rows), count, 0, _vp(offsets), None, 0, C.byref(t)) == 0
    assert t.value == 0 and offsets.tolist() == [0] * (count + 1)
