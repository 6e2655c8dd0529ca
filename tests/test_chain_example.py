"""examples/chain.c — pins from plain C: a 12-link chain on a world pin and a box dragged by a world pin that follows a cursor."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "chain")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "chain.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_chain_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_chain_example_holds_together_and_follows_the_cursor(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"chain: 13 pins after 600 steps, largest anchor separation ([0-9.]+)", r.stdout)
    assert m and float(m.group(1)) < 2.5, r.stdout
    assert "the pin schedule was built 1 time(s)" in r.stdout
