"""One World::Update on the device and on the oracle World in lockstep, and the byte comparison of the two (the pattern of
test_body_edits_gpu.py: the oracle's solver replays the device's schedule)."""
import numpy as np


def compare(pw, ow, step):
    assert pw.counts() == (len(ow.bodies()), len(ow.manifolds()), len(ow.contact_points()), len(ow.joints())), "step %d" % step
    assert pw.manifolds.tobytes() == ow.manifolds().tobytes(), "manifolds differ at step %d" % step
    assert pw.contactJoints.tobytes() == ow.joints().tobytes(), "joints differ at step %d" % step
    assert pw.bodies.tobytes() == ow.bodies().tobytes(), "bodies differ at step %d" % step
    m = ow.manifolds()
    first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    assert pw.contactPoints[live].tobytes() == ow.contact_points()[live].tobytes(), "contact points differ at step %d" % step


def step(oracle, pw, ow, cfg, dt):
    """pw.Update and the same step of the oracle World; the oracle's arrays are fetched anew (they move when it grows)."""
    pw.Update(dt, cfg)
    ow.pre_solve(dt)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(dt)
