"""examples/snap.c — breakable joints from plain C: the bridge's hangers under a break limit, crates dropped until they snap."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "snap")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "snap.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_snap_example_compiles(tmp_path, built_lib):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_snap_example_snaps_hangers_and_drops_the_deck(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    events = re.findall(r"step +(\d+): hanger (\d+) of plank (\d+) snapped: it transmitted ([0-9.]+), its limit allows ([0-9.]+)", r.stdout)
    assert events, r.stdout
    assert all(float(t) >= float(limit) for _, _, _, t, limit in events)
    steps = [int(e[0]) for e in events]
    assert steps == sorted(steps) and len({e[2] for e in events}) == len(events), "every plank's hanger snaps at most once, in step order"
    m = re.search(r"snap: (\d+) of 8 hangers snapped, (\d+) hold", r.stdout)
    assert m and int(m.group(1)) == len(events) and int(m.group(1)) + int(m.group(2)) == 8, r.stdout
