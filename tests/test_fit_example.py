"""examples/fit.c — the marble emitter that looks first: a marble is spawned above the funnel only when phx_world_query_circles says its
slot is free, and a circle cast says how far the next one can drop."""
import re
import subprocess

import pytest

import fit_example


def test_fit_example_compiles_and_refuses_a_negative_step_count(tmp_path, built_lib):
    exe = fit_example.build(tmp_path)
    r = subprocess.run([exe, "-1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr                    # (before any device call: the same with and without a GPU)


@pytest.mark.gpu
def test_marbles_are_spawned_only_into_a_free_slot(tmp_path, built_lib):
    exe = fit_example.build(tmp_path)
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spawned into an occupied slot" not in r.stderr
    m = re.search(r"fit: (\d+) marbles spawned, (\d+) requests refused", r.stdout)
    assert m and int(m.group(1)) + int(m.group(2)) == 600, r.stdout
    # a marble needs about 14 steps to fall its own height out of the slot: a spawn every 14 or so steps, never two in a row
    assert 20 <= int(m.group(1)) <= 60, r.stdout
    assert len(re.findall(r"the slot is free", r.stdout)) == int(m.group(1))
    m = re.search(r"touches body (\d+) after t = ([0-9.e+-]+), normal \((\S+), (\S+)\)", r.stdout)
    assert m, r.stdout
    # the drop goes down the middle of the funnel (from y = 200; the slot is at y = 100, the walls' lower ends near y = 50, 24 apart) and
    # ends on the tray's floor (its top at y = 2: t = 195) or on a marble lying there or on its way down
    assert 100.0 < float(m.group(2)) <= 195.0, r.stdout
    assert float(m.group(4)) > 0.0, "the normal points up, against the drop: %s" % r.stdout
