"""examples/bullet.c — continuous bodies from plain C: marbles at 120 units/s pass a thin wall and a wedge's thin foot when they are
discrete, and are stopped at both, on the wedge's slope itself, when they are continuous."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "bullet")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "bullet.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_bullet_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = _build(tmp_path)
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        pytest.skip("a GPU is present: covered by the gpu test")
    r = subprocess.run([exe, "30"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_discrete_marbles_tunnel_and_continuous_ones_do_not(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "30"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"bullet: discrete: (\d+) of 8 beyond the wall, (\d+) of 8 beyond the wedge after 30 steps; 0 passes, 0 clamps", r.stdout)
    assert m and int(m.group(1)) == 8 and int(m.group(2)) == 8, r.stdout
    m = re.search(r"bullet: continuous: 0 of 8 beyond the wall, 0 of 8 beyond the wedge after 30 steps; 30 passes, (\d+) clamps", r.stdout)
    assert m and int(m.group(1)) >= 16, r.stdout
    assert "sweep: 16 hits in the first continuous step" in r.stdout
    walls = re.findall(r"body (\d+) stopped by body 0 at t = ([0-9.]+), normal \(-1\.0000, -?0\.0000\)", r.stdout)
    assert [int(b) for b, _ in walls] == list(range(2, 10)) and all(abs(float(t) - (0.275 - 0.2 / 64.0 / 2.0)) < 2e-4 for _, t in walls), r.stdout
    slopes = re.findall(r"body (\d+) stopped by body 1 at t = ([0-9.]+), normal \(0\.4472, 0\.8944\)", r.stdout)
    assert [int(b) for b, _ in slopes] == list(range(10, 18)) and all(abs(float(t) - (0.15 - 0.2 / 64.0 / 2.0)) < 2e-4 for _, t in slopes), r.stdout
