"""examples/logs.c — capsule bodies from plain C: a dozen logs dropped onto a shelf between two posts, and a capsule that topples from its end."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "logs")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "logs.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_logs_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
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
def test_logs_pile_up_and_the_post_topples(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"logs: 13 capsules after 600 steps; (\d+) of 12 logs at rest, 0 lost", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 10, r.stdout
    m = re.search(r"pile: (\d+) manifolds with two points, (\d+) with one", r.stdout)
    assert m and int(m.group(1)) >= 2 and int(m.group(1)) + int(m.group(2)) >= 12, r.stdout      # every log rests on something; the bottom ones on a face
    m = re.search(r"post: \|sin\(angle\)\| ([0-9.]+), its centre at height ([0-9.]+)", r.stdout)
    assert m and float(m.group(1)) < 0.1 and abs(float(m.group(2)) - 5.5) < 2.0, r.stdout
