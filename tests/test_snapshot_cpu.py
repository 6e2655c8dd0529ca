"""The snapshot blob on the host (include/phyx_amd.h SNAPSHOTS; no GPU needed): phx_snapshot_blob_pack against tests/snapshot_spec.py
byte for byte, every rule of phx_snapshot_blob_check with one mutated blob each, the capacity protocol, and the device entry points
without a device.  (The golden files oracle_solver_stack2x10.npz / reference_lockstep.npz carry solver inputs and digests, not the four
arrays of a world state, so the states here are hand-made: tests/snapshot_cases.py.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

import snapshot_cases as cases
import snapshot_spec as spec
from phyx_amd import PhxError, Snapshot
from phyx_amd._lib import PHX_ERR_CAPACITY, PHX_ERR_INVALID, PHX_ERR_NO_DEVICE, PHX_OK


def _check(lib, blob):
    return lib.phx_snapshot_blob_check(blob, len(blob))


@pytest.mark.parametrize("name", sorted(cases.STATES))
def test_pack_equals_spec(built_lib, name):
    """Each state with each column NULL / given and the baseline explicit / NULL: the library's blob is the specification's, and both
    validators accept it."""
    b, m, c, j = cases.STATES[name]()
    n = len(b)
    f, mt, fl = cases.columns(n)
    explicit = np.array([[0, 1], [1, 2]], dtype=np.int32) if n >= 3 else np.zeros((0, 2), dtype=np.int32)
    for use_f, use_m, use_fl, use_b in itertools.product((False, True), repeat=4):
        kw = dict(filters=f if use_f else None, materials=mt if use_m else None, flags=fl if use_fl else None, baseline=explicit if use_b else None)
        want = spec.pack(b, m, c, j, **kw)
        got = Snapshot.pack(b, m, c, j, **kw)
        assert got == want, (name, use_f, use_m, use_fl, use_b)
        assert spec.check(want) is None
        assert _check(built_lib, got) == PHX_OK
        assert len(got) % 16 == 0


def test_null_baseline_is_the_touching_set(built_lib):
    b, m, c, j = cases.state_three_bodies()
    assert spec.touching(m).tolist() == [[0, 1], [0, 2]]                  # (the manifold without a live point is not touching)
    assert Snapshot.pack(b, m, c, j) == spec.pack(b, m, c, j, baseline=[[0, 1], [0, 2]])


@pytest.mark.parametrize("name", sorted(cases.mutations()))
def test_validator_names_every_broken_rule(built_lib, name):
    good = cases.three_body_blob()
    assert _check(built_lib, good) == PHX_OK and spec.check(good) is None
    bad = cases.mutations(good)[name]
    assert spec.check(bad) is not None, "the mutation must break the specification's rule too"
    assert _check(built_lib, bad) == PHX_ERR_INVALID
    assert b"snapshot blob" in built_lib.phx_last_error()
    with pytest.raises(PhxError):
        Snapshot.check_bytes(bad)


def test_validator_survives_short_and_empty_input(built_lib):
    good = cases.three_body_blob()
    for k in (0, 1, 8, 127, 128, 129, len(good) // 2):
        assert _check(built_lib, good[:k]) == PHX_ERR_INVALID
    assert built_lib.phx_snapshot_blob_check(None, 0) == PHX_ERR_INVALID
    assert _check(built_lib, good + b"\0" * 16) == PHX_ERR_INVALID          # longer than the header says


def test_pack_rejects_a_state_set_state_would_reject(built_lib):
    b, m, c, j = cases.state_three_bodies()
    j = j.copy(); j["body2"][0] = 2
    with pytest.raises(PhxError):
        Snapshot.pack(b, m, c, j)


def test_capacity(built_lib):
    from phyx_amd.api import _ptr
    b, m, c, j = cases.state_three_bodies()
    want = spec.pack(b, m, c, j)
    args = (_ptr(b), len(b), _ptr(m), len(m), _ptr(c), len(c), _ptr(j), len(j), None, None, None, None, 0)
    n = C.c_size_t(0)
    buf = C.create_string_buffer(len(want))
    assert built_lib.phx_snapshot_blob_pack(*args, buf, len(want) - 1, C.byref(n)) == PHX_ERR_CAPACITY
    assert n.value == len(want)
    n = C.c_size_t(0)
    assert built_lib.phx_snapshot_blob_pack(*args, None, 0, C.byref(n)) == PHX_ERR_CAPACITY and n.value == len(want)
    assert built_lib.phx_snapshot_blob_pack(*args, buf, len(want), C.byref(n)) == PHX_OK and buf.raw == want


def test_null_handles_are_invalid(built_lib):
    n = C.c_size_t(0)
    v = C.c_int32(0)
    assert built_lib.phx_world_save(None, None) == PHX_ERR_INVALID
    assert built_lib.phx_world_load(None, None) == PHX_ERR_INVALID
    assert built_lib.phx_snapshot_counts(None, C.byref(v), None, None, None) == PHX_ERR_INVALID
    assert built_lib.phx_snapshot_blob_bytes(None, C.byref(n)) == PHX_ERR_INVALID
    assert built_lib.phx_snapshot_export(None, None, 0) == PHX_ERR_INVALID
    assert built_lib.phx_snapshot_import(None, None, 0) == PHX_ERR_INVALID
    built_lib.phx_snapshot_destroy(None)


def test_snapshot_create_fails_loudly_without_gpu(built_lib):
    """In the manner of test_abi.py: no device, no snapshot, no fallback."""
    if built_lib.phx_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert built_lib.phx_snapshot_create(C.byref(h), 0) == PHX_ERR_NO_DEVICE
    assert not h.value
    assert b"no CPU fallback" in built_lib.phx_last_error()
    with pytest.raises(PhxError):
        Snapshot()
