"""Solver inputs built to land exactly on the capacity constants that choose a solve's kernel path (tests/test_path_edges_cpu.py checks
every construction with the host builder, tests/test_path_edges_gpu.py solves them on the device).

Construction technique.  A unit is one joint (contact point 2m) or two joints on one body pair (contact points 2m / 2m+1: a leader and
its follower, csrc/schedule.h UNITS).  A STAR whose dynamic hub carries d units is a clique of d units, so first fit gives it classes
0 .. d-1 whatever the priority order; class c of a set of disjoint stars therefore holds one unit of every star of degree > c, and the
leaders per class are any non-increasing sequence L.  Making every unit of some stars two-joint units sets the followers per class F the
same way (F non-increasing, F[c] - F[c+1] <= L[c] - L[c+1]).  A PATH along consecutive body indices gives the partitioned components their
level-0 classes: under the parity-major priority its links with an even lower body take class 0 (a perfect matching of a part's 512
bodies: 256 units), the odd ones class 1."""
import numpy as np

from test_solver_gpu import _random_state

# csrc/solver_kernels.h, csrc/solver.hip, csrc/schedule.h, csrc/island_view.h, csrc/schedule_kernels.h
TAIL_T, TAIL_CLASSES_MAX = 1024, 64
SOLVE_BLOCK, COLOUR_GRID_MAX = 64, 8192          # k_solve_colour: grid min(div_up(leaders, 64), 8192)
GRID_ITEMS = SOLVE_BLOCK * COLOUR_GRID_MAX       # = 256 * 2048 (grid_for): 524 288 items per grid pass
PART_BODIES, PARTS_T, PARTS_CLASS_STRIDE = 512, 256, 64
ISL_T, ISL_B, ISL_T_BIG, ISL_B_BIG = 256, 768, 512, 1024
COLOUR_B_MAX_JOINTS, BIN_CHUNK = 1024, 64


def units_state(seed, nb, units, static=(), shallow=False):
    """Solver input of `units` = rows (body a, body b, two joints?) over nb bodies (`static`: indices made static); the joint array is
    shuffled, contact point ids 2m / 2m+1 per unit m, plausible random masses, offsets, normals and warm-start impulses (_random_state).
    `shallow`: every body at the origin and every contact within the displacement pass's dead zone but four, which are 2.05 deep: the
    displacement sweeps stop being productive after a few sweeps, before the iteration count (4 of 6 in tail_of_3, both arithmetic forms)."""
    rng = np.random.default_rng(seed)
    units = np.asarray(units, dtype=np.int64).reshape(-1, 3)
    nu = len(units)
    two = units[:, 2] != 0
    nj = nu + int(two.sum())
    bodies, cps, joints = _random_state(rng, nb, 2 * nu, 0.0)
    st = np.asarray(static, dtype=np.int64)
    for f in ("inv_mass", "inv_inertia"):
        bodies[f][st] = 0.0
    for f in ("velocity", "displacing_velocity"):
        for n in ("x", "y"):
            if f in bodies.dtype.names:
                bodies[f][n][st] = 0.0
    bodies["angular_velocity"][st] = 0.0
    joints = joints[:nj].copy()
    u = np.arange(nu)
    unit = np.concatenate([u, u[two]])
    cp = np.concatenate([2 * u, 2 * u[two] + 1])
    pos = rng.permutation(nj)
    joints["body1"][pos], joints["body2"][pos] = units[unit, 0], units[unit, 1]
    joints["contact_point_index"][pos] = cp
    if shallow:
        bodies["pos"]["x"] = bodies["pos"]["y"] = 0.0
        r = np.random.default_rng(1)
        for d in ("delta1", "delta2"):
            cps[d]["x"] = r.uniform(-0.5, 0.5, len(cps))
            cps[d]["y"] = r.uniform(-0.5, 0.5, len(cps))
        k = np.arange(len(cps)) % (len(cps) // 4) == 0
        cps["delta1"]["x"][k] = cps["delta1"]["y"][k] = 0.0
        cps["delta2"]["x"][k], cps["delta2"]["y"][k] = 2.05 * cps["normal"]["x"][k], 2.05 * cps["normal"]["y"][k]
    return bodies, cps, joints


def star_units(leaders, followers=None, first=0, spoke=None):
    """Disjoint stars whose classes hold leaders[c] units, followers[c] of them two-joint units (default none): per degree d, L[d-1] - L[d]
    stars, F[d-1] - F[d] of them two-joint.  Bodies from `first` on: hub, then its spokes — or every spoke the body `spoke` (a static body:
    no conflict through it).  -> (units, next free body)"""
    L = list(leaders) + [0]
    F = list(followers if followers is not None else [0] * len(leaders)) + [0]
    assert all(L[c] >= L[c + 1] and F[c] >= F[c + 1] and F[c] - F[c + 1] <= L[c] - L[c + 1] for c in range(len(L) - 1))
    rows, b = [], first
    for d in range(len(L) - 1, 0, -1):
        n, n2 = L[d - 1] - L[d], F[d - 1] - F[d]
        if n == 0:
            continue
        if spoke is None:
            hub = b + np.arange(n) * (d + 1)
            sp = hub[:, None] + 1 + np.arange(d)[None, :]
            b += n * (d + 1)
        else:
            hub = b + np.arange(n)
            sp = np.full((n, d), spoke)
            b += n
        two = np.repeat((np.arange(n) < n2).astype(np.int64), d)
        rows.append(np.stack([np.repeat(hub, d), sp.ravel(), two], axis=1))
    return (np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)), b


def tail_first_class(leaders, first=0):
    """csrc/solver.hip tail_first_class restated: the first class of the trailing run of classes of at most TAIL_T leaders (at most
    TAIL_CLASSES_MAX of them) not before `first`, or the class count if that run is shorter than two classes."""
    ncol = len(leaders)
    t = ncol
    while t > first and leaders[t - 1] <= TAIL_T and ncol - (t - 1) <= TAIL_CLASSES_MAX:
        t -= 1
    return t if ncol - t >= 2 else ncol


def class_counts(order, offs, joints):
    """(leaders, followers) per class of a schedule: a follower is the odd contact point of a unit (every odd id here is one)."""
    foll = (joints["contact_point_index"][order] & 1).astype(np.int64)
    n = np.diff(offs)
    f = np.add.reduceat(foll, offs[:-1]) if len(order) else np.zeros(0, np.int64)
    f = np.where(n > 0, f, 0)
    return n - f, f


# ---- the tail (k_solve_tail): ISLAND_SINGLE, every joint in the HBM group ------------------------------------------------------------
# name -> (leaders per class, followers per class, stars on static spokes (leaders, followers) or None, designed first tail class)
TAIL_CASES = {
    # two classes of exactly TAIL_T leaders behind one of TAIL_T + 1; every tail leader has a follower (followers == leaders)
    "exact_1024_behind_1025": ([1025, 1024, 1024], [1024, 1024, 1024], None, 1),
    # a tail of two classes (even nclass) and of three (odd nclass); followers 0 in the last class
    "tail_of_2": ([1500, 700, 300], [900, 300, 0], None, 1),
    "tail_of_3": ([1500, 700, 300, 40], [900, 300, 40, 0], None, 1),
    # one qualifying trailing class only: no tail launch
    "single_trailing_class": ([1500, 1000], [1000, 500], None, 2),
    # more than TAIL_CLASSES_MAX trailing tiny classes (a star of degree 70: > 64 colours, the host builder): the tail capped at 64
    "over_64_trailing": ([1100] + [2] * 69, [500] + [1] * 69, None, 70 - 64),
    # tail units on static bodies shared by every class: stars whose spokes are all static body 0
    "static_spokes": ([1300, 400, 400, 400], [600, 200, 200, 200], ([20, 20, 20, 20], [10, 10, 10, 10]), 1),
}


def tail_state(name, seed=1, shallow=False):
    leaders, followers, on_static, _ = TAIL_CASES[name]
    first = 1
    rows = []
    if on_static is not None:
        sl, sf = on_static
        s_rows, first = star_units(sl, sf, first, spoke=0)
        rows.append(s_rows)
        leaders = [a - b for a, b in zip(leaders, sl + [0] * (len(leaders) - len(sl)))]
        followers = [a - b for a, b in zip(followers, sf + [0] * (len(followers) - len(sf)))]
    r, nb = star_units(leaders, followers, first)
    rows.append(r)
    return units_state(seed, nb, np.concatenate(rows), static=[0], shallow=shallow)


# ---- the grid caps: one class of GRID_ITEMS + 1 leaders, one of GRID_ITEMS, every unit two joints --------------------------------------
GRID_LEADERS = [GRID_ITEMS + 1, GRID_ITEMS]


def grid_state(seed=3):
    r, nb = star_units(GRID_LEADERS, GRID_LEADERS, 1)
    return units_state(seed, nb, r, static=[0])


# ---- partitioned components (k_solve_parts_ahead at level 0, k_solve_parts at level 1) ----------------------------------------
def unit_part(a, b, nb):
    """csrc/schedule.h unit_part restated for two dynamic bodies: the part a unit is interior to, or -1."""
    P = (nb + PART_BODIES - 1) // PART_BODIES
    if a // PART_BODIES == b // PART_BODIES:
        return a // PART_BODIES
    h = PART_BODIES // 2
    return P + (a + h) // PART_BODIES if (a + h) // PART_BODIES == (b + h) // PART_BODIES else -1


def parts_units(nb, level1, star0=0, dense0=0):
    """One partitioned component over bodies [0, nb), every unit two joints: a path along the bodies of every level-0 part (its links
    (i, i+1) inside the part: class 0 = the links with an even lower body, a perfect matching of a full part's 512 bodies = 256 units,
    class 1 = the other 255) and, across the level-0 boundary 512 (k + 1), stars with the degrees level1[k], hub on one side, spokes on
    the other (level-1 interior units; level-1 class c of that part = its stars of degree > c).  star0 > 0: a star of that degree inside
    part 0 besides (level-0 interior: more level-0 classes); dense0 > 0: the links of part 0 repeated until it holds dense0 interior units."""
    rows = []
    P = (nb + PART_BODIES - 1) // PART_BODIES
    for p in range(P):
        lo, hi = p * PART_BODIES, min((p + 1) * PART_BODIES, nb)
        a = np.arange(lo, hi - 1)
        rows.append(np.stack([a, a + 1, np.ones_like(a)], axis=1))
    if dense0:
        a = np.arange(0, min(PART_BODIES, nb) - 1)
        extra = dense0 - len(a) - (star0 or 0)
        rep = np.resize(a, extra)
        rows.append(np.stack([rep, rep + 1, np.ones_like(rep)], axis=1))
    if star0:
        hub = 300
        sp = np.setdiff1d(np.arange(PART_BODIES), [hub])[:star0]
        rows.append(np.stack([np.full(star0, hub), sp, np.ones(star0, np.int64)], axis=1))
    for k, degrees in enumerate(level1):
        edge = (k + 1) * PART_BODIES
        left, right = list(range(edge - PART_BODIES // 2, edge)), list(range(edge, min(edge + PART_BODIES // 2, nb)))
        for d in degrees:
            hub_side, spoke_side = (left, right) if len(right) - d >= len(left) - 1 else (right, left)
            hub = hub_side.pop(0)
            for _ in range(d):
                rows.append(np.array([[min(hub, spoke_side[0]), max(hub, spoke_side[0]), 1]]))
                spoke_side.pop(0)
    return np.concatenate(rows)


def level1_degrees(sizes):
    """star degrees whose classes hold sizes[c] units (non-increasing)"""
    L = list(sizes) + [0]
    return [d for d in range(len(sizes), 0, -1) for _ in range(L[d - 1] - L[d])]


# name -> (bodies, level-1 class sizes per boundary, star0, dense0); NB_PARTS is not a multiple of 512: a partial last level-0 part
NB_PARTS = 3 * PART_BODIES + 300
PARTS_CASES = {
    # level 0: full parts' class 0 = 256 units (every lane of k_solve_parts_ahead); level 1: a part of 256 units in all (200 + 56: every
    # unit owned by a lane), one of 267 (200 + 57 + 10: the 257th unit in the middle of class 1, swept by k_solve_parts' loop past the owned
    # units, and a class behind it whose `before` passes PARTS_T: the clamp max(PARTS_T - before, 0)), one of 3; the last level-0 part
    # holds 300 bodies
    "lanes_256_257": (NB_PARTS, [[200, 56], [200, 57, 10], [2, 1]], 0, 0),
    # a level-0 star of degree 70 in part 0: more than PARTS_CLASS_STRIDE = 64 interior classes (no part tables: every class a launch)
    "over_64_interior_classes": (2 * PART_BODIES, [[30, 10]], 70, 0),
    # part 0 holds exactly CP_MAXU = 3072 interior units (the device's part colouring) and 3073 (past it: the host builder)
    "cp_maxu_3072": (2 * PART_BODIES, [[30, 10]], 0, 3072),
    "cp_maxu_3073": (2 * PART_BODIES, [[30, 10]], 0, 3073),
}


def parts_state(name, seed=5):
    nb, sizes, star0, dense0 = PARTS_CASES[name]
    return units_state(seed, nb, parts_units(nb, [level1_degrees(s) for s in sizes], star0, dense0))


# ---- LDS group shapes (ISLAND_MULTIPLE): one path component of `units` units, the first `two` of them two joints --------------------
# name -> (units, two-joint units, expected: "small" | "big" | "hbm")
LDS_CASES = {
    "units_256": (256, 256, "small"),          # ISL_T units (and 2 * ISL_T joints): the small shape's capacity exactly
    "units_257": (257, 0, "big"),              # one unit more: the 512-lane shape
    "units_512_joints_1024": (512, 512, "big"),    # ISL_T_BIG units, COLOUR_B_MAX_JOINTS joints: the big shape's capacity exactly
    "units_513": (513, 0, "hbm"),              # one unit more: the HBM group
    "units_513_joints_1025": (513, 512, "hbm"),    # (1025 joints need 513 units: the joint and the unit edge coincide)
}


def lds_state(name, seed=7):
    u, two, _ = LDS_CASES[name]
    a = np.arange(u)
    rows = np.stack([a, a + 1, (a < two).astype(np.int64)], axis=1)
    # and a few small components beside it (a bin holds several)
    extra = np.arange(20) * 2 + u + 1
    rows = np.concatenate([rows, np.stack([extra, extra + 1, np.ones_like(extra)], axis=1)])
    return units_state(seed, u + 1 + 40, rows)
