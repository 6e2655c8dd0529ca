"""examples/marbles.c — round bodies from plain C: marbles dropped through a funnel of static boxes into a tray, and a circle on a motor."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "marbles")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "marbles.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_marbles_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_marbles_fall_through_the_funnel_and_the_wheel_turns(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"marbles: 37 circles after 600 steps; (\d+) of 36 marbles through the funnel, (\d+) at rest, 0 lost", r.stdout)
    assert m, r.stdout
    # the funnel's gap (24) is four marbles wide and its walls are steeper (0.7 rad) than friction 0.3 holds a rolling disc on: none stays up
    assert int(m.group(1)) == 36, r.stdout
    m = re.search(r"wheel: (-?[0-9.]+) rad/s on its motor \(set 4.0\), its centre ([0-9.]+) from the axle", r.stdout)
    assert m, r.stdout
    assert abs(float(m.group(1)) - 4.0) < 1e-2 and float(m.group(2)) < 0.05, r.stdout
