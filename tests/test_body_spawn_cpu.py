"""Spawning bodies between steps (include/phyx_amd.h, phx_world_add_bodies / phx_world_set_inverse_masses): what can be checked
without a GPU — the entry points refuse a null handle, the Python wrappers refuse bad input before any C call, the scene-dict form
maps static / pinned to the values add_scene uses, and examples/emitter.c builds and fails loudly without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from phyx_amd import scenes
from phyx_amd.api import pinned_inv_inertia

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    spawn = np.array([[0.0, 0.0, 0.0, 1.0, 1.0]], dtype=np.float32)
    idx = np.array([0], dtype=np.int32)
    vals = np.zeros((1, 2), dtype=np.float32)
    first = C.c_int32(0)
    assert L.phx_world_add_bodies(None, spawn.ctypes.data_as(C.c_void_p), 1, C.byref(first)) == -1
    assert L.phx_world_add_bodies(None, None, 0, None) == -1
    assert L.phx_world_set_inverse_masses(None, idx.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), 1) == -1
    assert L.phx_world_set_inverse_masses(None, None, None, 0) == -1
    assert b"null handle" in L.phx_last_error()


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world(lib=None):
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = lib if lib is not None else _NoC(), None
    return w


@pytest.mark.parametrize("spawn", [np.zeros((3, 4), dtype=np.float32), np.zeros((3, 6), dtype=np.float32), np.zeros(5, dtype=np.float32),
                                   np.zeros((2, 5, 1), dtype=np.float32)])
def test_add_bodies_refuses_bad_shapes(spawn):
    with pytest.raises(ValueError):
        _world().add_bodies(spawn)


@pytest.mark.parametrize("spawn", [np.zeros((3, 5), dtype=np.int32), np.zeros((3, 5), dtype=bool), [["a"] * 5], 7])
def test_add_bodies_refuses_bad_dtypes(spawn):
    with pytest.raises((TypeError, ValueError)):
        _world().add_bodies(spawn)


def test_add_bodies_refuses_bad_scene_dicts():
    sc = scenes.stack(2, 2)
    for bad in ({k: v for k, v in sc.items() if k != "sy"},
                dict(sc, px=sc["px"][:-1]),
                dict(sc, static=np.zeros(2, dtype=bool)),
                dict(sc, angle=np.array(["x"] * len(sc["px"])))):
        with pytest.raises((TypeError, ValueError)):
            _world().add_bodies(bad)


def test_set_inverse_masses_refuses_bad_arrays():
    w = _world()
    with pytest.raises(TypeError):
        w.set_inverse_masses(np.array([0.0]), np.zeros((1, 2), dtype=np.float32))        # indices must be integers
    with pytest.raises(TypeError):
        w.set_inverse_masses([0], np.zeros((1, 2), dtype=np.int32))                    # values must be floats
    with pytest.raises(ValueError):
        w.set_inverse_masses([0, 1], np.zeros((2, 3), dtype=np.float32))               # (K, 2)
    with pytest.raises(ValueError):
        w.set_inverse_masses([0, 1], np.zeros((1, 2), dtype=np.float32))


class _Recorder:
    """Records the two spawn calls instead of running them (a world of `n` bodies before the call)."""

    def __init__(self, n):
        self.n, self.rows, self.edits = n, None, []

    def phx_world_add_bodies(self, h, spawn, count, first):
        self.rows = np.ctypeslib.as_array(C.cast(spawn, C.POINTER(C.c_float)), shape=(count, 5)).copy() if count else np.zeros((0, 5), np.float32)
        C.cast(first, C.POINTER(C.c_int32))[0] = self.n
        return 0

    def phx_world_set_inverse_masses(self, h, bodies, values, count):
        idx = np.ctypeslib.as_array(C.cast(bodies, C.POINTER(C.c_int32)), shape=(count,)).copy()
        val = np.ctypeslib.as_array(C.cast(values, C.POINTER(C.c_float)), shape=(count, 2)).copy()
        self.edits.append((idx, val))
        return 0


def test_scene_dict_maps_static_and_pinned_as_add_scene_does():
    sc = scenes.stack(3, 2)
    sc["sx"][2], sc["sy"][2] = 7.5, 3.25
    sc["pinned"] = np.zeros(len(sc["px"]), dtype=bool)
    sc["pinned"][[2, 4]] = True
    sc["static"][4] = True                                  # static and pinned: pinned wins, as in add_scene (set after set_static)
    rec = _Recorder(10)
    idx = _world(rec).add_bodies(sc)
    assert idx.tolist() == list(range(10, 10 + len(sc["px"])))
    want = np.stack([sc["px"], sc["py"], sc["angle"], sc["sx"], sc["sy"]], axis=1).astype(np.float32)
    assert rec.rows.tobytes() == want.tobytes()
    assert len(rec.edits) == 1
    bodies, values = rec.edits[0]
    assert bodies.tolist() == [10, 12, 14]
    assert values.tolist() == [[0.0, 0.0], [0.0, pinned_inv_inertia(7.5, 3.25)], [0.0, pinned_inv_inertia(5.0, 5.0)]]
    # the float formula of add_scene (ref: main.cpp:176-177 on AddBody's mass, RigidBody.h:15-36)
    mass = np.float32(1e-5) * (np.float32(7.5) * np.float32(3.25))
    assert pinned_inv_inertia(7.5, 3.25) == float(np.float32(1.0) / (mass * (np.float32(7.5) * np.float32(7.5) + np.float32(3.25) * np.float32(3.25))))
    # a dict without static / pinned bodies makes no inverse-mass call
    rec = _Recorder(0)
    plain = {k: v for k, v in scenes.stack(2, 2).items() if k != "static"}
    _world(rec).add_bodies(plain)
    assert rec.edits == []


def test_emitter_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = str(tmp_path / "emitter")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "emitter.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        pytest.skip("a GPU is present: covered by the gpu test")
    r = subprocess.run([exe, "10", "2", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
