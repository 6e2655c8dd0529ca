"""examples/fold.c — collision exclusions from plain C: a folded chain dropped on its end falls through itself under one negative group
and piles up on itself with only its neighbours excluded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "fold")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "fold.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    return exe


def test_fold_example_compiles(tmp_path, built_lib):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_fold_example_folds_onto_itself(tmp_path, built_lib):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"fold: shared group -1: (\d+) neighbour manifolds, (\d+) other link-link manifolds", r.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) == 0, r.stdout
    m = re.search(r"fold: neighbours excluded: (\d+) neighbour manifolds, (\d+) other link-link manifolds", r.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) > 0, r.stdout
