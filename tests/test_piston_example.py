"""examples/piston.c — slider joints from plain C: a crank-slider whose piston stays on its line and runs a stroke of twice the crank
radius, an elevator that stops at its stops and whose motor the loop reverses, a box on a spring slider."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The same scene through tests/slider_spec.py's step_free (nothing touches: no contacts) at 16 sweeps on the CPU, 600 steps: the piston
# ran from 10.99367 to 17.00987, a stroke of 6.01621 against 2 x 3 (the pins' Baumgarte slack at the dead centres), 9.2e-5 off its line
# at the most; the elevator stayed within [0, 20] exactly (20 is 80 steps of 15 / 60), stood at 20 before the reversal and at 0 at the
# end; the box sagged 1.26652 = g / (2 pi 2)^2.  The bounds are twice what was observed beyond the ideal; the elevator's is the stop plus
# one step's travel, which is what a limit that engages the step after it is passed allows.
STROKE_SLACK = 2.0 * 0.01621
OFF_LINE = 2.0 * 9.2e-5
ONE_STEP = 15.0 / 60.0


def _build(tmp_path):
    exe = str(tmp_path / "piston")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "piston.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_piston_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_piston_example_slides_stops_and_springs(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"piston: 3 sliders after 600 steps; the piston ran from ([0-9.]+) to ([0-9.]+), a stroke of ([0-9.]+) \(crank radius 3.0\), "
                  r"and left its line by ([0-9.]+) at the most", r.stdout)
    assert m, r.stdout
    assert float(m.group(4)) < OFF_LINE, "the piston stays on its line: " + r.stdout
    assert abs(float(m.group(3)) - 6.0) < STROKE_SLACK, "the stroke is twice the crank radius: " + r.stdout
    m = re.search(r"elevator: between (-?[0-9.]+) and (-?[0-9.]+) \(stops 0 and 20\), at (-?[0-9.]+) before the reversal and at (-?[0-9.]+) at the end", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) > -ONE_STEP and float(m.group(2)) < 20.0 + ONE_STEP, "the elevator stops at its limits: " + r.stdout
    assert abs(float(m.group(3)) - 20.0) < 1e-3 and abs(float(m.group(4))) < 1e-3, r.stdout
    m = re.search(r"suspension: sags (-?[0-9.]+) \(g / w\^2 = (-?[0-9.]+)\)", r.stdout)
    assert m and abs(float(m.group(1)) - float(m.group(2))) < 1e-3, r.stdout
    assert "built 1 time(s)" in r.stdout
