"""examples/wind.c — force fields from plain C: boxes drop through a wind zone into a drag pool on a shelf, then a blast scatters them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "wind")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "wind.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_wind_example_compiles(tmp_path, built_lib):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_wind_example_blows_slows_and_scatters(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "4", "3", "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"wind: the boxes landed (-?[\d.]+) downwind", r.stdout)
    assert m and float(m.group(1)) > 0.0, r.stdout
    m = re.search(r"pool: (\d+) boxes entered at ([\d.]+) and were at ([\d.]+) 8 frames later", r.stdout)
    assert m and int(m.group(1)) == 12 and float(m.group(3)) < float(m.group(2)), r.stdout
    m = re.search(r"blast at frame 240: (\d+) of 12 boxes moved", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout
    assert re.search(r"wind: 300 frames, 300 field passes", r.stdout), r.stdout
