"""Parity at the sizes the kernels were built for (MI355X): solver inputs whose joint indices pass k_build_bin's packed sort key,
a World past 2^22 joints in the 512-lane shape, the benchmark's 200k-box world through its merged and its loosened regime, and
cfg 4's million-box world step.  As everywhere else, the oracle replays the device's own schedule and every byte must agree; each
test also asserts that it reached the regime it is about, so that none can pass vacuously."""
import os

import numpy as np
import pytest

import phyx_amd
from phyx_amd import scenes, Configuration
from test_solver_gpu import _device_solve, _oracle_in_device_order, _random_state
from test_world_gpu import _lockstep

pytestmark = pytest.mark.gpu

# the settled regime's solve, as the bench runs it (bench.py cfg 2)
BENCH_CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)


def _chain_state(seed, sizes, limit, rewired=0.0, single=0.1):
    """A synthetic solver input of chains: component c is a path of sizes[c] dynamic bodies with a unit on every link — two joints
    (contact points 2m / 2m+1) or, for a fraction `single` of the links, one (2m alone); every 4th chain (every 3rd if `rewired`)
    also rests its first body on the static body 0 by a one-joint unit, so that the static body sits in many bins.  (Paths need at most three
    classes a bin: the host builder allows 65 000 classes in all, and this input has ~2e4 bins.)  The joint array is shuffled,
    but the leaders of the two-joint units stay below `limit` while every other joint (single units, followers) may land anywhere:
    a unit that k_build_bin's sort loses is then noticed only if it has a follower (its `joints_here` check rejects the bin and
    the whole build falls back to the host builder, which would hide a wrong sort), so the units whose leaders pass the limit are
    the single ones.  `rewired` > 0: the next step of a world whose contacts moved — about that fraction of the chains trades its
    bodies with a neighbour and more chains rest on the static body (another joint count: like a World step, the solve knows
    that the schedule must be rebuilt before it runs, which is when the rebuild may take the speculative path)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    nc = len(sizes)
    first = 1 + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    c = np.repeat(np.arange(nc), sizes - 1)                                  # the links: (a, a + 1) of chain c
    a = np.arange(len(c)) - np.repeat(np.cumsum(sizes - 1) - (sizes - 1), sizes - 1)
    b = a + 1
    st = np.arange(0, nc, 3 if rewired else 4)
    c = np.concatenate([c, st]); a = np.concatenate([a, np.zeros(len(st), np.int64)]); b = np.concatenate([b, np.zeros(len(st), np.int64)])
    pair = np.concatenate([rng.random(len(c) - len(st)) >= single, np.zeros(len(st), bool)])
    nu, npair = len(c), int(pair.sum())
    nj = nu + npair
    nb = 1 + int(sizes.sum())
    bodies, cps, joints = _random_state(rng, nb, 2 * nu, 0.0)              # (bodies, contact points and impulses: plausible values)
    bodies["inv_mass"][0] = bodies["inv_inertia"][0] = 0.0
    bodies["velocity"]["x"][0] = bodies["velocity"]["y"][0] = 0.0
    joints = joints[:nj].copy()
    # joint positions: the two-joint units' leaders below `limit`, every other joint in the positions left
    lead_pos = rng.choice(limit, npair, replace=False)
    free = np.ones(nj, dtype=bool)
    free[lead_pos] = False
    rest_pos = rng.permutation(np.flatnonzero(free))
    if rewired:
        # chains 2i and 2i + 1 of one length trade their bodies (along each path the body indices keep increasing, as in a stack's
        # column: the device's one labelling pass of a speculative rebuild converges on such paths, on arbitrary ones it may not)
        r = np.random.default_rng(seed + 1)
        pick = 2 * np.flatnonzero(r.random(nc // 2) < rewired)
        pick = pick[sizes[pick] == sizes[pick + 1]]
        first[pick], first[pick + 1] = first[pick + 1], first[pick].copy()
    b1 = first[c] + a
    b2 = np.where(np.arange(nu) < nu - len(st), first[c] + b, 0)             # (the static units' second body: body 0)
    u = np.arange(nu)
    pu = u[pair]
    su = u[~pair]
    pos = np.concatenate([lead_pos, rest_pos])
    unit = np.concatenate([pu, su, pu])                                      # leaders of pairs, single units, followers
    cp = np.concatenate([2 * pu, 2 * su, 2 * pu + 1])
    joints["body1"][pos], joints["body2"][pos] = b1[unit], b2[unit]
    joints["contact_point_index"][pos] = cp
    return bodies, cps, joints


def _record_paths_parity(oracle, seed, sizes, limit, lanes):
    """Two solves on one handle — the long way (recoloured == 1), then the next step (_chain_state's `rewired`), binned
    speculatively (recoloured == 2): the device schedule is a permutation of the joints, equals the host builder's, sits in
    LDS groups of the expected shape only, and the solve equals the oracle's replay of it byte for byte."""
    cfg = Configuration(phyx_amd.SOLVE_SCALAR, phyx_amd.ISLAND_MULTIPLE, 2, 2)
    os.environ["PHX_SCHEDULE_BUILDER"] = "host"
    try:
        host = phyx_amd.Solver(0)
    finally:
        del os.environ["PHX_SCHEDULE_BUILDER"]
    dev = phyx_amd.Solver(0)
    for rewired, want in ((0.0, 1), (0.1, 2)):
        state = _chain_state(seed, sizes, limit, rewired)
        nj = len(state[2])
        assert nj > limit
        db, dj, ds, _, dst = _device_solve(dev, state, cfg)
        _, lane = dev.lanes()
        print("%d joints, %d bins, lanes up to %d, %d classes, recoloured %d" % (nj, ds.lds_groups, lane.max(), dst.colour_count, dst.recoloured))
        assert dst.recoloured == want
        assert np.array_equal(np.sort(ds.order), np.arange(nj, dtype=ds.order.dtype))
        assert int(ds.groups[ds.lds_groups]) == nj and dst.lds_islands > 0      # every unit in a workgroup's bin ...
        assert (lane.max() >= 256) == (lanes == 512)                            # ... of the expected shape
        hb, hj, hs, _, hst = _device_solve(host, state, cfg)
        assert np.array_equal(hs.order, ds.order) and np.array_equal(hs.colours, ds.colours)
        assert np.array_equal(hs.groups, ds.groups) and hs.lds_groups == ds.lds_groups
        assert hb.tobytes() == db.tobytes() and hj.tobytes() == dj.tobytes()
        del hb, hj, hs
        ob_, oj, ost = _oracle_in_device_order(oracle, state, ds, None, cfg, oracle.STAG_COLOUR_SYNC)
        assert db.tobytes() == ob_.tobytes() and dj.tobytes() == oj.tobytes()
        assert (dst.impulse_iterations, dst.displacement_iterations) == (ost.impulse_iterations, ost.displacement_iterations)
        del state, db, dj, ob_, oj


def test_record_paths_past_the_packed_key_limit(oracle, built_lib):
    """k_build_bin sorts a bin's units by (leader joint, lane) as ONE 32-bit key only while every joint index fits 31 - 8 bits (256
    lanes).  37 400 chains of 128 bodies (127 or 128 units each, two to a bin) give ~9.0 M joints, past 2^23, so that the bins mix
    leaders on both sides of the limit; both builds from the joints' records (the long way, then speculative binning) must sort
    by two words here."""
    _record_paths_parity(oracle, 7, np.full(37400, 128), 1 << 23, 256)


def test_record_paths_past_the_packed_key_limit_512_lanes(oracle, built_lib):
    """The same at the 512-lane shape (ISL_T_BIG), whose packed key holds joint indices below 2^22 only: every tenth chain has
    300 bodies (more units than the small shape holds), the others 128 — 16 000 chains, ~4.4 M joints."""
    _record_paths_parity(oracle, 8, np.where(np.arange(16000) % 10 == 0, 300, 128), 1 << 22, 512)


def test_world_rebuilds_from_the_manifolds_past_2_22_joints(oracle, built_lib):
    """The World's rebuild from the manifolds in the 512-lane shape at more than 2^22 joints — k_build_bin's two-word sort on that
    path: 4400 columns of 500 boxes (each column one island of 500 units: the roomier shape), ~4.4 M joints, in lockstep with the
    oracle, and at least one of the steps' rebuilds came from the manifolds."""
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 10, 10)
    seen = []

    def look(pw, step):
        _, lane = pw.solver.lanes()
        seen.append((pw.counts()[3], int(lane.max()), pw.solver.groups()[1]))
    pw, ow = _lockstep(oracle, scenes.stack(4400, 500), 10, cfg, check_every=1, on_step=look)
    lite, full = pw.build_counts()
    print("joints, top lane, bins per step:", seen, "rebuilds from the manifolds / the joints:", (lite, full))
    assert all(nj > (1 << 22) and top >= 256 for nj, top, _ in seen), seen
    assert lite >= 1, (lite, full)


def test_bench_world_merged_and_loosened_lockstep(oracle, built_lib):
    """The benchmark's world — stack(1000, 200) under the bench's configuration — in lockstep with the oracle through step 104: the
    columns merge into one island of 6 - 8e5 joints at about step 28 (partitioned: k_solve_parts_ahead over several hundred parts,
    k_jp_walk_one colouring the boundary units, the two-launch flattening pass k_cc_compress_window / k_cc_compress) and loosen again
    by about step 100 (hundreds of workgroup-sized islands beside the big one, whose trailing tiny classes k_solve_tail sweeps in one
    launch: 81 sweep launches per solve with it, 241 without).  Every byte is compared every 10th step and at every step of 57 - 61
    and 100 - 104.  Measured on the MI355X: 783 parts at step 60, 418 - 431 workgroup islands and 81 sweep launches per solve at
    steps 100 - 104; one rocprofv3 --kernel-trace --stats run of this test counted 1540 launches of k_solve_parts_ahead, 740 of
    k_solve_tail, 76 of k_jp_walk_one, 112 of k_cc_compress_window and 107 of k_build_bin."""
    seen = {}

    def look(pw, step):
        if step == 60 or step >= 100:
            st = pw.solver.stats()
            seen[step] = (st.lds_islands,) + tuple(pw.solver.partition())
    _lockstep(oracle, scenes.stack(1000, 200), 105, BENCH_CFG, check_every=10, check_at=list(range(57, 62)) + list(range(100, 105)), on_step=look)
    print("lds_islands, interior classes, parts, sweep launches:", seen)
    _, ki, parts, _ = seen[60]
    assert ki > 0 and parts >= 600, seen[60]                    # merged: one partitioned island (the bench recorded 783 parts)
    for step in range(100, 105):
        islands, ki, parts, launches = seen[step]
        assert islands >= 200 and ki > 0 and parts > 0, (step, seen[step])      # loosened: hundreds of LDS islands beside the big one
        assert 0 < launches <= 120, (step, seen[step])           # the trailing classes in k_solve_tail's one launch (241 without it)


def test_cfg4_world_step_lockstep(oracle, built_lib):
    """cfg 4's world step — stack(10000, 100), a million bodies, the bench's configuration — in lockstep with the oracle, every byte
    of every step: ~5 000 bins built by k_build_bin, more workgroups than are resident at once (the island kernel's residency rounds,
    gated by the topology hash: ISL_GATED), the million-body side-stream labelling."""
    cu = phyx_amd.device_info(0)["compute_units"]
    seen = []

    def look(pw, step):
        st = pw.solver.stats()
        seen.append((st.lds_islands, pw.solver.groups()[1]))
    _lockstep(oracle, scenes.stack(10000, 100), 4, BENCH_CFG, check_every=1, on_step=look)
    print("lds_islands, bins per step:", seen, "compute units:", cu)
    for islands, bins in seen:
        assert islands >= 4000 and bins >= 4000, seen
        assert bins > 4 * cu, (bins, cu)                         # at most 4 island workgroups per CU: several residency rounds
