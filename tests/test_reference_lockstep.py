"""The oracle World against the reference's own World, stepped together (tests/reference_runs.py): every byte of bodies,
manifolds, live contact points and joints after every step, in all twelve solve / island modes on the long runs, and in two
modes on the scenes of test_world_gpu.py, the reference's demo scenes and BASELINE config 2.

Each run is checked against the committed per-step digests of the strict reference build (tests/golden/reference_lockstep.npz),
so the check never depends on the reference being present; where oracle/_ref/libphyx_ref_full_strict.so exists the library is
also stepped alongside and compared field by field.  The reference takes its parallel pair path; its serial one is pinned as a
known deviation by test_serial_pair_path_deviation_is_where_it_was."""
import collections
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle import binding as ob
import reference_runs as rr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIGESTS = os.path.join(HERE, "golden", "reference_lockstep.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(DIGESTS)


def _live():
    return os.path.exists(ob.ref_full_path("strict"))


def test_every_run_has_digests(gold):
    for name, s, i in rr.RUNS:
        assert gold[rr.run_key(name, s, i)].shape == (rr.SCENES[name][1], len(rr.FIELDS), 16)
    assert len(rr.RUNS) >= 2 * 12


@pytest.mark.parametrize("name,solve_mode,island_mode", rr.RUNS, ids=[rr.run_key(*r) for r in rr.RUNS])
def test_oracle_steps_with_the_reference(oracle, gold, name, solve_mode, island_mode):
    make, steps, _ = rr.SCENES[name]
    want = gold[rr.run_key(name, solve_mode, island_mode)]
    scene = make()
    ow = rr.make_world("oracle", scene)
    rw = rr.make_world("strict", scene) if _live() else None
    joints = 0
    for step in range(steps):
        ow.update(rr.DT, solve_mode, island_mode, rr.ITERS, rr.ITERS)
        st = rr.state(ow)
        if rw is not None:
            rw.update(rr.DT, solve_mode, island_mode, rr.ITERS, rr.ITERS)
            rs = rr.state(rw)
            for f in rr.FIELDS:
                assert st[f].tobytes() == rs[f].tobytes(), "%s differ from the live reference after step %d" % (f, step + 1)
        got = rr.digest(st)
        for k, f in enumerate(rr.FIELDS):
            assert (got[k] == want[step, k]).all(), "%s differ from the reference's digest after step %d" % (f, step + 1)
        joints += len(st["joints"])
    assert joints > 0


def _pair_count(world, pair):
    m = world.manifolds()
    return int(((m["body1"] == pair[0]) & (m["body2"] == pair[1])).sum())


def test_serial_pair_path_deviation_is_where_it_was(oracle, gold):
    """DESIGN.md §9 item 2 against the reference itself.  On its serial pair path (World::Update with 0 workers) the reference's
    manifoldMap.insert re-admits a pair it already holds when a tombstone lies ahead of it in the probe chain (ref:
    base/DenseHash.h:152), and the manifold list then holds that pair twice.  Its parallel path, which the oracle and the device
    restate, filters with contains() and holds it once.  In falling1k (Scalar, Single) the two paths first differ at the step on
    record, and only by that duplicate; if a change to the reference or to the oracle moves it, the deviation must be looked at again."""
    first = int(gold["serial_first_step"])
    pair = tuple(int(v) for v in gold["serial_duplicate_pair"])
    serial = gold["serial_digests"]
    sm, im = rr.SERIAL_MODE
    parallel = gold[rr.run_key(rr.SERIAL_SCENE, sm, im)][:len(serial)]
    differs = np.flatnonzero((serial != parallel).any(axis=(1, 2)))
    assert len(differs) and int(differs[0]) + 1 == first, "the committed serial digests first differ at step %d" % (differs[0] + 1)
    # the oracle holds the pair exactly once at that step, and matches the parallel path's digest there
    scene = rr.SCENES[rr.SERIAL_SCENE][0]()
    ow = rr.make_world("oracle", scene)
    for _ in range(first):
        ow.update(rr.DT, sm, im, rr.ITERS, rr.ITERS)
    assert _pair_count(ow, pair) == 1
    assert (rr.digest(rr.state(ow)) == parallel[first - 1]).all()
    m = ow.manifolds()
    assert len(set(zip(m["body1"].tolist(), m["body2"].tolist()))) == len(m)
    if not _live():
        return
    # the live reference: the serial path reproduces its digests, holds the pair twice at `first` and nowhere before
    rw = rr.make_world("strict", scene, ob.PAIRS_SERIAL)
    for step in range(1, len(serial) + 1):
        rw.update(rr.DT, sm, im, rr.ITERS, rr.ITERS)
        assert (rr.digest(rr.state(rw)) == serial[step - 1]).all(), "serial path, step %d" % step
        m = rw.manifolds()
        twice = [p for p, c in collections.Counter(zip(m["body1"].tolist(), m["body2"].tolist())).items() if c > 1]
        if step < first:
            assert not twice, step
        elif step == first:
            assert twice == [pair] and len(m) == len(ow.manifolds()) + 1


def test_loading_the_native_libraries_keeps_the_fp_environment():
    """Loading a library linked with -ffast-math runs crtfastmath.o's constructor, which sets MXCSR's flush-to-zero and
    denormals-are-zero bits for the whole process, and every later oracle computation in it would silently flush denormals.
    oracle/Makefile compiles the fast libraries with -ffast-math and links them without it; this loads every one of them (and the
    oracle) in a fresh interpreter and requires MXCSR, and denormal arithmetic, to be as they were."""
    libs = [os.path.join(ROOT, "oracle", "liboracle.so")]
    ob.baseline_lib("fast"), ob.baseline_lib("strict"), ob.lib()
    libs += [os.path.join(ROOT, "oracle", "libcpubaseline_%s.so" % k) for k in ("fast", "strict")]
    ref = os.path.join(ROOT, "oracle", "_ref")
    if os.path.isdir(ref):
        libs += sorted(os.path.join(ref, f) for f in os.listdir(ref) if f.endswith(".so"))
    assert all(os.path.exists(p) for p in libs)
    probe = textwrap.dedent("""
        import ctypes, ctypes.util, sys
        import numpy as np
        libm = ctypes.CDLL(ctypes.util.find_library("m"))
        def mxcsr():
            env = (ctypes.c_uint8 * 64)()
            assert libm.fegetenv(env) == 0
            return int.from_bytes(bytes(env[28:32]), "little")     # glibc x86-64 fenv_t: the x87 environment, then __mxcsr
        def denormals():
            d = np.array([1e-39], dtype=np.float32)
            return bool(d[0] * np.float32(1.0) != 0) and bool(d[0] > 0)
        before, ok = mxcsr(), denormals()
        for path in sys.argv[1:]:
            ctypes.CDLL(path)
            after = mxcsr()
            print(path, hex(before), hex(after), denormals())
            assert after & 0x8040 == before & 0x8040 and denormals() == ok, path
        assert ok
    """)
    r = subprocess.run([sys.executable, "-c", probe] + libs, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
