"""IntegrateVelocity (ref: World.cpp:39-55) is one device function with three callers (csrc/body_view.h integrate_velocity); which of them
a step runs depends on whether it is the world's first update, on phase timing and on PHX_NO_SPLIT_SORT.  Every caller against the oracle
World, byte for byte (tests/integrate_paths.py)."""
import os
import subprocess
import sys

import pytest

import integrate_paths

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm", ["default", "phase_timing", "no_split_sort"])
def test_integrate_velocity_on_every_path(oracle, built_lib, arm):
    """default: step 1 k_build_keys<true>, steps 2-3 k_keys_buckets<true, 2>; phase_timing: the unfused k_integrate_velocity;
    no_split_sort: k_build_keys<true> on every step.  Each without and with pending accelerations."""
    if arm == "no_split_sort":
        p = subprocess.run([sys.executable, os.path.abspath(integrate_paths.__file__)], env=dict(os.environ, PHX_NO_SPLIT_SORT="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-2000:]
        return
    for accel in (False, True):
        integrate_paths.lockstep(oracle, arm == "phase_timing", accel)
