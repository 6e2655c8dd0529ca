"""examples/ramp.c — convex polygon bodies from plain C: boxes, marbles and a hexagon come down a static wedge into a trapezoid tray, and a
ray finds the slope and its normal."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "ramp")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "ramp.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_ramp_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_everything_comes_down_the_ramp_into_the_tray(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"ramp: 3 polygons after 600 steps; (\d+) of 7 bodies in the tray, 0 lost", r.stdout)
    assert m and int(m.group(1)) >= 6, r.stdout
    m = re.search(r"face: (\d+) manifolds with two points on the ramp after 10 steps", r.stdout)
    assert m and int(m.group(1)) >= 3, r.stdout                                  # the three boxes lie on the face; the hexagon may have begun to tumble
    m = re.search(r"ray: down at x = -28 hits body 0 at height ([0-9.]+), normal \(([0-9.]+), ([0-9.]+)\)", r.stdout)
    assert m and abs(float(m.group(1)) - 21.0) < 0.01 and abs(float(m.group(2)) - 0.4472) < 1e-3 and abs(float(m.group(3)) - 0.8944) < 1e-3, r.stdout
