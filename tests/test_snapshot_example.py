"""examples/rollback.c — device snapshots from plain C: a ring of saved worlds, a rollback every 20th frame, bit-equal re-simulation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "rollback")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rollback.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_rollback_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = _build(tmp_path)
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        pytest.skip("a GPU is present: covered by the gpu test")
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_rollback_example_resimulates_bit_for_bit(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rollback: 3 rollbacks, 18 re-simulated frames, all equal to the first pass" in r.stdout
    assert r.stdout.count("equals the first pass") == 3
