"""The specification of collision filters (include/phyx_amd.h, COLLISION FILTERS): the rule that decides whether a pair may collide,
and the state that phx_world_set_state must be given to make the world that phx_world_set_collision_filters leaves.  Plain numpy; the
device is held to it byte for byte (tests/test_collision_filters_gpu.py)."""
import numpy as np

from phyx_amd.api import collision_filter_dtype

DEFAULT = (1, 0xFFFFFFFF, 0)


def filters(n, category=1, mask=0xFFFFFFFF, group=0):
    """n filters of collision_filter_dtype, each field a scalar or one value per body."""
    f = np.zeros(n, dtype=collision_filter_dtype)
    f["category"], f["mask"], f["group"] = category, mask, group
    return f


def should_collide(fa, fb):
    """The rule, elementwise over filter records (or arrays of them): a shared non-zero group decides alone (positive: collide,
    negative: never); otherwise each body's mask must meet the other's category."""
    ga, gb = np.asarray(fa["group"], dtype=np.int64), np.asarray(fb["group"], dtype=np.int64)
    shared = (ga == gb) & (ga != 0)
    ca, ma = np.asarray(fa["category"], dtype=np.uint64), np.asarray(fa["mask"], dtype=np.uint64)
    cb, mb = np.asarray(fb["category"], dtype=np.uint64), np.asarray(fb["mask"], dtype=np.uint64)
    masks = ((ma & cb) != 0) & ((mb & ca) != 0)
    return np.where(shared, ga > 0, masks)


def pair_passes(filt, body1, body2):
    """should_collide for the body pairs (body1[k], body2[k]) under the per-body filters `filt`."""
    b1, b2 = np.asarray(body1, dtype=np.int64), np.asarray(body2, dtype=np.int64)
    return should_collide(filt[b1], filt[b2]).astype(bool)


def drop(state, filt):
    """(bodies, manifolds, contact points, joints) after the filters `filt` (one per body) drop the manifolds whose pair fails:
      - bodies unchanged;
      - the manifolds whose pair passes, in their old order, point_index = 2 * new manifold index;
      - their two contact-point slots; a live slot's solver_index follows its joint (-1 if the joint goes, unchanged if it is outside
        [0, joint count)), dead slots byte for byte;
      - the joints of kept manifolds, in order, contact_point_index = 2 * new manifold + old % 2.
    Returns (state, dropped manifold count)."""
    bodies, manifolds, cps, joints = state
    nm, nj = len(manifolds), len(joints)
    mkeep = pair_passes(filt, manifolds["body1"], manifolds["body2"]) if nm else np.zeros(0, dtype=bool)
    mnew = np.full(nm, -1, dtype=np.int64)
    mnew[mkeep] = np.arange(int(mkeep.sum()))

    jkeep = mkeep[joints["contact_point_index"] // 2] if nj else np.zeros(0, dtype=bool)
    jnew = np.full(nj, -1, dtype=np.int32)
    jnew[jkeep] = np.arange(int(jkeep.sum()), dtype=np.int32)

    out_m = manifolds[mkeep].copy()
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
    return (bodies.copy(), out_m, out_c, out_j), int(nm - mkeep.sum())
