"""The specification of collision exclusions (include/phyx_amd.h, COLLISION EXCLUSIONS): the set of unordered body pairs that never
collide, its membership test, the state that phx_world_set_state must be given to make the world that
phx_world_add_collision_exclusions leaves, and the set's way through a removal of bodies.  Plain numpy; the device is held to it byte
for byte (tests/test_exclusions_gpu.py)."""
import numpy as np


def normalize(pairs):
    """The set as the world stores and returns it: (n, 2) int32 rows {min(a, b), max(a, b)}, distinct, ascending by (lo, hi)."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if not len(p):
        return np.zeros((0, 2), dtype=np.int32)
    assert (p[:, 0] != p[:, 1]).all(), "a pair names one body twice"
    lo, hi = np.minimum(p[:, 0], p[:, 1]), np.maximum(p[:, 0], p[:, 1])
    return np.unique(np.stack([lo, hi], axis=1), axis=0).astype(np.int32).reshape(-1, 2)


def _keys(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return (np.minimum(a, b) << 32) | np.maximum(a, b)


def excluded(pairs, body1, body2):
    """Membership: whether the unordered pairs {body1[k], body2[k]} are in the set `pairs` (a bool array)."""
    s = normalize(pairs)
    return np.isin(_keys(body1, body2), _keys(s[:, 0], s[:, 1]))


def union(pairs, more):
    return normalize(np.concatenate([normalize(pairs), normalize(more)]))


def difference(pairs, less):
    s = normalize(pairs)
    return s[~excluded(less, s[:, 0], s[:, 1])] if len(s) else s


def drop(state, pairs):
    """(bodies, manifolds, contact points, joints) after the set `pairs` drops the manifolds whose pair it holds — the compaction
    filter_spec.drop states, with "the pair is not in the set" as the keep rule:
      - bodies unchanged;
      - the manifolds whose pair is not excluded, in their old order, point_index = 2 * new manifold index;
      - their two contact-point slots; a live slot's solver_index follows its joint (-1 if the joint goes, unchanged if it is outside
        [0, joint count)), dead slots byte for byte;
      - the joints of kept manifolds, in order, contact_point_index = 2 * new manifold + old % 2.
    Returns (state, dropped manifold count)."""
    bodies, manifolds, cps, joints = state
    nm, nj = len(manifolds), len(joints)
    mkeep = ~excluded(pairs, manifolds["body1"], manifolds["body2"]) if nm else np.zeros(0, dtype=bool)
    mnew = np.cumsum(mkeep) - 1                                             # (read at kept manifolds only)
    jkeep = mkeep[joints["contact_point_index"] // 2] if nj else np.zeros(0, dtype=bool)
    jnew = np.where(jkeep, np.cumsum(jkeep) - 1, -1).astype(np.int32)
    kept = np.flatnonzero(mkeep)

    out_m = manifolds[kept].copy()
    out_m["point_index"] = 2 * np.arange(len(kept), dtype=np.int32)
    out_c = cps[np.stack([2 * kept, 2 * kept + 1], axis=1).reshape(-1)].copy()
    for slot in range(len(out_c)):
        si = int(out_c["solver_index"][slot])
        if slot % 2 < int(out_m["point_count"][slot // 2]) and 0 <= si < nj:
            out_c["solver_index"][slot] = jnew[si]
    out_j = joints[jkeep].copy()
    if len(out_j):
        cpi = out_j["contact_point_index"]
        out_j["contact_point_index"] = 2 * mnew[cpi // 2] + cpi % 2
    return (bodies.copy(), out_m, out_c, out_j), int(nm - len(kept))


def remap(pairs, new):
    """The set after a removal of bodies with the remap new[] (-1: removed; increasing on the kept bodies): pairs with a removed body
    go, the others are renumbered — lo < hi and the order both survive."""
    s = normalize(pairs)
    new = np.asarray(new, dtype=np.int64)
    moved = new[s.astype(np.int64)] if len(s) else np.zeros((0, 2), dtype=np.int64)
    return moved[(moved >= 0).all(axis=1)].astype(np.int32).reshape(-1, 2)
