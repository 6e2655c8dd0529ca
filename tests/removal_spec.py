"""The specification of removing bodies from a world (include/phyx_amd.h, phx_world_remove_bodies): the state that
phx_world_set_state must be given to make the world a removal leaves.  Plain numpy on the four arrays state() returns; the device is
held to it byte for byte (tests/test_body_removal_gpu.py)."""
import numpy as np


def new_index(body_count, removed):
    """new[i] = the new index of old body i, or -1 if it is removed."""
    keep = np.ones(body_count, dtype=bool)
    keep[np.asarray(removed, dtype=np.int64)] = False
    new = np.full(body_count, -1, dtype=np.int32)
    new[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    return new


def outside(bodies, box):
    """The bodies whose AABB does not overlap the closed box (min.x, min.y, max.x, max.y), as float32 comparisons."""
    lo, hi = np.float32(box[0]), np.float32(box[2])
    bl, bh = np.float32(box[1]), np.float32(box[3])
    inside = ((bodies["aabb_min"]["x"] <= hi) & (bodies["aabb_max"]["x"] >= lo) &
              (bodies["aabb_min"]["y"] <= bh) & (bodies["aabb_max"]["y"] >= bl))
    return np.flatnonzero(~inside).astype(np.int32)


def filter(state, removed):
    """(bodies, manifolds, contact points, joints) after removing the bodies `removed` from `state`, and new[]:
      - bodies not removed, in their old order, each record unchanged but `index` = its new position;
      - manifolds whose two bodies are both kept, in order, bodies remapped, point_index = 2 * new manifold index;
      - the two contact-point slots of each kept manifold; a live slot's solver_index follows its joint (-1 if the joint goes,
        unchanged if it is outside [0, joint count)), dead slots byte for byte;
      - joints whose manifold is kept, in order, bodies remapped, contact_point_index = 2 * new manifold + old % 2."""
    bodies, manifolds, cps, joints = state
    nb, nm, nj = len(bodies), len(manifolds), len(joints)
    new = new_index(nb, removed)

    out_b = bodies[new >= 0].copy()
    out_b["index"] = np.arange(len(out_b), dtype=np.uint32)

    mkeep = np.zeros(nm, dtype=bool)
    if nm:
        mkeep = (new[manifolds["body1"]] >= 0) & (new[manifolds["body2"]] >= 0)
    mnew = np.full(nm, -1, dtype=np.int64)
    mnew[mkeep] = np.arange(int(mkeep.sum()))

    jkeep = mkeep[joints["contact_point_index"] // 2] if nj else np.zeros(0, dtype=bool)
    jnew = np.full(nj, -1, dtype=np.int32)
    jnew[jkeep] = np.arange(int(jkeep.sum()), dtype=np.int32)

    out_m = manifolds[mkeep].copy()
    out_m["body1"] = new[out_m["body1"]]
    out_m["body2"] = new[out_m["body2"]]
    out_m["point_index"] = 2 * np.arange(len(out_m), dtype=np.int32)

    slots = np.stack([2 * np.flatnonzero(mkeep), 2 * np.flatnonzero(mkeep) + 1], axis=1).reshape(-1)
    out_c = cps[slots].copy()
    if len(out_c):
        live = np.repeat(out_m["point_count"], 2) > np.tile(np.arange(2), len(out_m))
        si = out_c["solver_index"]
        follow = live & (si >= 0) & (si < nj)
        si[follow] = jnew[si[follow]]

    out_j = joints[jkeep].copy()
    if len(out_j):
        cpi = out_j["contact_point_index"]
        out_j["contact_point_index"] = 2 * mnew[cpi // 2] + cpi % 2
        out_j["body1"] = new[out_j["body1"]]
        out_j["body2"] = new[out_j["body2"]]
    return (out_b, out_m, out_c, out_j), new


def set_state_problems(state):
    """What phx_world_set_state would refuse in `state` (its checks, csrc/world_state.hip World::set_state), plus the record index
    invariant AddBody sets up (ref: World.cpp:14); an empty list if none."""
    bodies, manifolds, cps, joints = state
    nb, nm = len(bodies), len(manifolds)
    out = []
    if len(cps) != 2 * nm:
        out.append("contact point count %d != 2 * %d manifolds" % (len(cps), nm))
    if not np.array_equal(bodies["index"], np.arange(nb, dtype=np.uint32)):
        out.append("body index != position")
    for i, m in enumerate(manifolds):
        if not (0 <= m["body1"] < nb and 0 <= m["body2"] < nb):
            out.append("manifold %d: body out of range" % i)
        if m["point_index"] != 2 * i or not 0 <= m["point_count"] <= 2:
            out.append("manifold %d: slots" % i)
    for j, q in enumerate(joints):
        c = int(q["contact_point_index"])
        if not 0 <= c < len(cps):
            out.append("joint %d: contact point out of range" % j)
            continue
        m = manifolds[c // 2]
        if q["body1"] != m["body1"] or q["body2"] != m["body2"]:
            out.append("joint %d: bodies differ from its manifold's" % j)
        if cps[c]["solver_index"] != j:
            out.append("joint %d: its contact point does not point back" % j)
    return out
