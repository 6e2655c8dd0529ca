"""examples/bridge.c — links from plain C: a pinned deck on rod hangers, a crate on a rope, a box on a spring that follows a cursor."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The same scene, the same cursor and 16 sweeps through tests/pin_spec.py and tests/link_spec.py (unit_spec.step_free: no contacts, and
# none forms in the example either), 600 steps on the CPU: the largest pin separation was 0.1704, the largest rod length error 0.0556.
# The bounds are twice those.
PIN_SEPARATION = 2.0 * 0.1704
ROD_ERROR = 2.0 * 0.0556


def _build(tmp_path):
    exe = str(tmp_path / "bridge")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "bridge.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_bridge_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_bridge_example_holds_together(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"bridge: 9 pins and 10 links after 600 steps, largest pin separation ([0-9.]+), largest rod length error ([0-9.]+)", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) < PIN_SEPARATION and float(m.group(2)) < ROD_ERROR, r.stdout
    assert "rope: slack yes, taut yes" in r.stdout
    assert "built 1 time(s)" in r.stdout
