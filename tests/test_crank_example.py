"""examples/crank.c — angle joints from plain C: a door that stops at its stop, a wheel on a motor whose speed the loop reverses, two
boxes welded by a pin plus a lock."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The same scene through the oracle's contacts and tests/angle_spec.py at 16 sweeps on the CPU, 600 steps: the door went to 0.5091 at
# the most and stood at 0.5000001, the wheel turned at exactly 4 and -4, the weld stayed at 0 (the lock is the last unit of its sweep
# and the two inertias are equal) while the pair swung 3.11 rad.  The door's bound is the stop plus twice the overshoot observed.
DOOR_WORST = 0.5 + 2.0 * 0.0091


def _build(tmp_path):
    exe = str(tmp_path / "crank")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "crank.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_crank_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_crank_example_stops_drives_and_welds(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"crank: 3 angles after 600 steps; the door went to ([0-9.]+) at the most and stands at (-?[0-9.]+) \(stop 0.5\)", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) < DOOR_WORST and abs(abs(float(m.group(2))) - 0.5) < 1e-3, r.stdout
    m = re.search(r"wheel: (-?[0-9.]+) rad/s before the reversal, (-?[0-9.]+) after; weld: bent ([0-9.]+) at the most while it swung ([0-9.]+)", r.stdout)
    assert m, r.stdout
    assert abs(float(m.group(1)) - 4.0) < 1e-3 and abs(float(m.group(2)) + 4.0) < 1e-3 and float(m.group(3)) < 1e-3 and float(m.group(4)) > 1.0, r.stdout
    assert "built 1 time(s)" in r.stdout
