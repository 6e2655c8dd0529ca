"""The specification of body flags and sensors (include/phyx_amd.h, BODY FLAGS / SENSORS): which manifolds are sensor manifolds, what the
state-changing calls do to the per-body flag words, and RefreshContactJoints (ref: World.cpp:72-149) with the one added rule.  Plain
numpy and Python loops — the shapes of the tests are tiny; the device is held to it byte for byte (tests/test_sensors_gpu.py), and with
every flag 0 it is the oracle World's own refresh byte for byte (tests/test_sensors_cpu.py).

tag_twin_* reconstruct the state just before RefreshContactJoints, which no getter shows: a twin world steps the same step with
friction_acc[k] = k + 1 written into its joints first, so that after the refresh a joint's tag says which old joint it was."""
import numpy as np

BODY_SENSOR = 1


def defaults(n):
    return np.zeros(n, dtype=np.uint32)


def sensor_manifolds(flags, manifolds):
    """Per manifold: is either of its bodies a sensor."""
    flags = np.asarray(flags, dtype=np.uint32)
    if not len(manifolds):
        return np.zeros(0, dtype=bool)
    b1, b2 = manifolds["body1"].astype(np.int64), manifolds["body2"].astype(np.int64)
    return ((flags[b1] | flags[b2]) & np.uint32(BODY_SENSOR)) != 0


def live_slots(manifolds):
    """The contact-point indices of every manifold's live slots, in manifold order, then slot order."""
    out = []
    for m in manifolds:
        out += [int(m["point_index"]) + k for k in range(int(m["point_count"]))]
    return np.asarray(out, dtype=np.int64)


def sensor_slots(flags, manifolds):
    """The live slots of the sensor manifolds."""
    return live_slots(manifolds[sensor_manifolds(flags, manifolds)]) if len(manifolds) else np.zeros(0, dtype=np.int64)


def refresh(manifolds, cps, joints, flags, stats=None):
    """RefreshContactJoints restated statement by statement: Reset; Match with the sensor rule in front of the reference's test (a live
    slot of a sensor manifold gets solver_index = -1 and nothing else happens for it); the reference's swap-remove Cleanup.  `cps` carry
    the solver_index they had when the reference's function would be entered, `joints` are the joints of the step before.  Returns new
    (cps, joints); the inputs stay as they are.  `stats` (a dict) receives matched / created / deleted."""
    cps = cps.copy()
    sensor = sensor_manifolds(flags, manifolds)
    J = [[int(j["contact_point_index"]), int(j["body1"]), int(j["body2"]), j["normal_acc"], j["friction_acc"]] for j in joints]
    matched = created = deleted = 0
    for j in J:                                                         # Reset
        j[0] = -1
    for mi in range(len(manifolds)):                                    # Match
        man = manifolds[mi]
        for k in range(int(man["point_count"])):
            cpi = int(man["point_index"]) + k
            if sensor[mi]:                                              # the added rule
                cps["solver_index"][cpi] = -1
                continue
            si = int(cps["solver_index"][cpi])
            if si < 0:
                cps["solver_index"][cpi] = len(J)
                J.append([cpi, int(man["body1"]), int(man["body2"]), np.float32(0), np.float32(0)])
                created += 1
            else:
                assert J[si][1] == int(man["body1"]) and J[si][2] == int(man["body2"])
                J[si][0] = cpi
                matched += 1
    i = 0
    while i < len(J):                                                   # Cleanup
        if J[i][0] < 0:
            J[i] = J[-1]
            J.pop()
            deleted += 1
        else:
            cps["solver_index"][J[i][0]] = i
            i += 1
    out = np.zeros(len(J), dtype=joints.dtype)
    for i, j in enumerate(J):
        out[i] = tuple(j)
    if stats is not None:
        stats.update(matched=matched, created=created, deleted=deleted)
    return cps, out


# ---- the tag twin ----------------------------------------------------------------------------------------------------------------------
def tags(count):
    """friction_acc of `count` joints as tags: joint k carries k + 1 (exact in float32 below 2^24)."""
    assert count < 2 ** 24
    return np.arange(1, count + 1, dtype=np.float32)


def tag_twin_reconstruct(manifolds, twin_cps, twin_joints, cps):
    """`cps` (a copy) with every live slot's solver_index set to what it was before the twin's refresh: the twin's joint of that slot
    carries tag t — old joint t - 1, or (t == 0) a joint the refresh made: -1.  Also returns, per twin joint, that old index."""
    old = twin_joints["friction_acc"].astype(np.int64) - 1
    out = cps.copy()
    for cpi in live_slots(manifolds):
        j = int(twin_cps["solver_index"][cpi])
        assert 0 <= j < len(twin_joints) and int(twin_joints["contact_point_index"][j]) == cpi, "the twin's slot and joint do not point at each other"
        out["solver_index"][cpi] = old[j]
    return out, old


# ---- the state transforms -----------------------------------------------------------------------------------------------------------
def spawn(flags, count):
    """add_body / add_bodies: new bodies get 0."""
    return np.concatenate([np.asarray(flags, dtype=np.uint32), defaults(count)])


def remove(flags, keep):
    """remove_bodies / remove_outside: the kept bodies' flags move with them, through new[] (kept order)."""
    return np.asarray(flags, dtype=np.uint32)[np.asarray(keep, dtype=bool)].copy()


def set_state(n):
    """phx_world_set_state: every flag is 0 again."""
    return defaults(n)


def valid(flags):
    """The values phx_world_set_body_flags accepts: no bit but BODY_SENSOR."""
    return (np.asarray(flags, dtype=np.uint32) & ~np.uint32(BODY_SENSOR)) == 0
