"""examples/rest.c — sleeping from plain C: boxes rain onto a shelf until the pile rests, then a dropped crate wakes the column it hits."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "rest")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rest.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_rest_example_compiles(tmp_path, built_lib):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_rest_example_rests_and_wakes_one_column(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "6", "3", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert re.search(r"rest: the pile rests after \d+ seconds", r.stdout), r.stdout
    m = re.search(r"the crate \(body 19\) woke((?: \d+)+)", r.stdout)
    assert m, r.stdout
    woke = [int(x) for x in m.group(1).split()]
    assert woke == [10, 11, 12], "the crate lands on the middle column (bodies 10 .. 12) and wakes exactly it"
    m = re.search(r"rest: (\d+) asleep now, (\d+) put to sleep and (\d+) woken in total", r.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) - int(m.group(3)) == 15, r.stdout
