"""Edits between steps and the O(count) gathers (include/phyx_amd.h, phx_world_add_accelerations ...): what can be checked without a
GPU — the entry points refuse a null handle, the Python wrappers refuse bad arrays before the C call, examples/drag.c builds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDITS = ("phx_world_add_accelerations", "phx_world_set_velocities", "phx_world_set_poses")


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    idx = np.array([0], dtype=np.int32)
    vals = np.zeros(6, dtype=np.float32)
    for name in EDITS:
        assert getattr(L, name)(None, idx.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), 1) == -1
        assert getattr(L, name)(None, None, None, 0) == -1
    out = np.zeros(128, dtype=np.uint8)
    assert L.phx_world_get_body_states(None, idx.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.phx_world_get_poses(None, vals.ctypes.data_as(C.c_void_p), 1) == -1
    assert L.phx_world_get_poses_device(None, None, 0) == -1
    assert b"null handle" in L.phx_last_error()


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with arrays the wrapper should have refused" % name)


def _world():
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = _NoC(), None
    return w


@pytest.mark.parametrize("method,width", [("add_accelerations", 3), ("set_velocities", 3), ("set_poses", 6)])
def test_wrappers_refuse_bad_arrays(method, width):
    w = _world()
    fn = getattr(w, method)
    good = np.zeros((2, width), dtype=np.float32)
    with pytest.raises(ValueError):
        fn([0, 1], np.zeros((3, width), dtype=np.float32))          # one row per index
    with pytest.raises(ValueError):
        fn([0, 1], np.zeros((2, width + 1), dtype=np.float32))      # row width
    with pytest.raises(ValueError):
        fn([0, 1], np.zeros(2 * width, dtype=np.float32))           # flat
    with pytest.raises(TypeError):
        fn([0, 1], good.astype(np.int32))                           # values must be floats
    with pytest.raises(TypeError):
        fn(np.array([0.0, 1.0]), good)                              # indices must be integers
    with pytest.raises(TypeError):
        fn(np.array([[0, 1]]), good)                                # ... in a 1-D array
    with pytest.raises(TypeError):
        fn(np.array([True, False]), good)
    with pytest.raises(ValueError):
        fn(np.array([0, 2 ** 40]), good)                            # beyond int32


def test_gather_wrappers_refuse_bad_arrays():
    w = _world()
    with pytest.raises(TypeError):
        w.body_states(np.array([0.5]))
    with pytest.raises(TypeError):
        w.body_states(np.zeros((2, 2), dtype=np.int32))
    w.counts = lambda: (3, 0, 0, 0)
    for bad in (np.zeros((3, 4), dtype=np.float64), np.zeros((2, 4), dtype=np.float32), np.zeros((4, 3), dtype=np.float32).T):
        with pytest.raises(ValueError):
            w.poses(out=bad)


def test_set_poses_angle_form_matches_add_body():
    """(K, 3) {x, y, angle} becomes the frame AddBody computes (ref: RigidBody.h:15-36): float angle + pi / 2, double cos / sin."""
    from phyx_amd.api import frame_from_angle
    for angle in (0.0, 0.3, -1.2, 3.0, 1e-7):
        a = np.float32(angle)
        q = np.float32(a + np.float32(1.570796))
        want = np.array([1.0, 2.0, np.cos(np.float64(a)), np.sin(np.float64(a)), np.cos(np.float64(q)), np.sin(np.float64(q))], dtype=np.float32)
        assert frame_from_angle(1.0, 2.0, angle).tobytes() == want.tobytes()


def _build(tmp_path):
    exe = str(tmp_path / "drag")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "drag.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_drag_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = _build(tmp_path)
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        pytest.skip("a GPU is present: covered by tests/test_body_edits_gpu.py")
    r = subprocess.run([exe, "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
