"""The narrowphase corpus: box pairs, each walked through a few phases, that between them take every arm of the oracle's
separating_axis / support points / generate_contacts / add_point / update_manifold (oracle/phx_oracle.h PHXO_T_*).

A case is two boxes and up to MAX_PHASES poses of both.  Case k owns bodies 2k and 2k + 1 and lives alone in cell k of a grid of
pitch PITCH (GRID cells to a row): half-extents are at most 12 and every pose stays within 50 of the cell's centre, so no box of one
case comes near a box of another.  Phase 1 is given as (x, y, angle) and built by add_scene; every phase is a 6-float frame
{pos.x, pos.y, xv.x, xv.y, yv.x, yv.y} in float32.  A case with fewer phases keeps its last pose.  A box with a zero half-extent has
no mass (RigidBody.h: invMass = 1 / (density * w * h)), so it is static: nothing here holds an infinity.

Deterministic, builds no files, imports nothing of the project.  tests/test_narrowphase_cpu.py proves on the CPU which labels the
corpus reaches; REQUIRED is the list every run must reach in at least MIN_CASES distinct cases, NOT_REQUIRED the rest, each with its
reason, and the test asserts that the corpus reaches none of those."""
import math

import numpy as np

PITCH = 128.0
GRID = 64
MAX_PHASES = 8
MIN_CASES = 4

REQUIRED = [
    "sep0", "sep1", "sep2", "sep3", "best0", "best1", "best2", "best3", "flip", "noflip",
    "sup1_edge_y_pos", "sup1_edge_y_neg", "sup1_edge_x_pos", "sup1_edge_x_neg",
    "sup1_vertex_pp", "sup1_vertex_pn", "sup1_vertex_np", "sup1_vertex_nn",
    "sup2_edge_y_pos", "sup2_edge_y_neg", "sup2_edge_x_pos", "sup2_edge_x_neg",
    "sup2_vertex_pp", "sup2_vertex_pn", "sup2_vertex_np", "sup2_vertex_nn",
    "collapse1", "collapse2", "vv_hit", "vv_miss", "ve_hit", "ve_miss", "ev_hit", "ev_miss",
    "ee_tc0", "ee_tc1", "ee_tc2", "ee_tc3", "ee_tc4",
    "ee_pick01", "ee_pick02", "ee_pick03", "ee_pick12", "ee_pick13", "ee_pick23",
    "append_slot0", "append_slot1", "append_slot2", "append_slot3", "merge_slot0", "merge_slot1", "merge_slot2",
    "merge_later_candidate", "equals_one_sided",
    "from0_to0", "from0_to1", "from0_to2", "from1_to0", "from1_to1", "from1_to2", "from2_to0", "from2_to1", "from2_to2",
    "keep_shift", "dead", "empty_alive",
]

# label -> why no input reaches it
NOT_REQUIRED = {
    "merge_slot3": "slot 3 exists only once the second, and last, add_point of an update has appended it (two cached points, slot 2 "
                   "appended by the first call): no call is left that could merge into it.  tools/narrowphase_search.py: 0 of 4 000 000 pairs",
    "overflow": "an update calls add_point at most twice, each call marks exactly one point merged, and the cached points start the "
                "update unmarked: never more than two merged points for two slots.  tools/narrowphase_search.py: 0 of 4 000 000 pairs",
}

F32 = np.float32
ONE_BELOW = float(np.nextafter(F32(1), F32(0)))
SMALL = [1.0, ONE_BELOW, 0.5, 0.25, 0.0]
QUARTER = float(F32(math.pi / 2))


def frame(x, y, angle):
    """The frame RigidBody's constructor gives a body at `angle` (ref: RigidBody.h:15-36, Coords2.h:10-17: the float angle and
    angle + 3.141592f / 2 go through the double cos / sin, then narrow to float)."""
    a = F32(angle)
    q = F32(a + F32(F32(3.141592) / F32(2.0)))
    return np.array([x, y, math.cos(float(a)), math.sin(float(a)), math.cos(float(q)), math.sin(float(q))], dtype=F32)


def tilted_frame(x, y, s, quarter_turns=0):
    """A frame whose xVector is (sqrt(1 - s^2), s) in float32 with s given exactly, turned by whole quarter turns (exact: components
    swap and change sign).  Against an axis-aligned box's (0, +-1) axis the dot is +-s exactly: the way onto the 0.1 threshold."""
    s = F32(s)
    c = F32(math.sqrt(1.0 - float(s) * float(s)))
    xv, yv = (c, s), (-s, c)
    for _ in range(quarter_turns % 4):
        xv, yv = yv, (-xv[0], -xv[1])
    return np.array([x, y, xv[0], xv[1], yv[0], yv[1]], dtype=F32)


def _ulps(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return float(v)


def threshold_angles():
    """float32 angles around asin(0.1) whose frame's sin lands a few ulps below, and on or a few ulps above, 0.1f: (below, above)."""
    tenth = F32(0.1)
    base = F32(math.asin(0.1))
    below, above = [], []
    for k in range(-12, 13):
        a = _ulps(base, k)
        s = frame(0, 0, a)[3]
        d = (int(s.view(np.int32)) - int(tenth.view(np.int32)))
        if -3 <= d < 0:
            below.append(a)
        elif 0 <= d <= 3:
            above.append(a)
    return below, above


class Case:
    """size: (2, 2) half-extents; static: (2,) bool; start: (2, 3) {x, y, angle} of phase 1, already placed; frames: (phases, 2, 6)."""

    def __init__(self, family, size, static, start, frames):
        self.family, self.size, self.static, self.start, self.frames = family, size, static, start, frames


class _Builder:
    def __init__(self):
        self.cases = []

    def add(self, family, size_a, size_b, start_a, start_b, later=(), swap=False):
        """start_*: (x, y, angle) relative to the cell's centre.  later: per phase (pose_a, pose_b), a pose being (x, y, angle), a
        6-float frame relative to the centre, or None for 'as in the phase before'.  swap: box B takes the lower body index."""
        k = len(self.cases)
        cx, cy = F32((k % GRID) * PITCH), F32((k // GRID) * PITCH)
        size = np.array([size_a, size_b], dtype=F32)
        assert size.min() >= 0 and size.max() <= 12
        poses = [(start_a, start_b)] + list(later)
        assert len(poses) <= MAX_PHASES
        frames = np.zeros((len(poses), 2, 6), dtype=F32)
        start = np.zeros((2, 3), dtype=F32)
        for p, pair in enumerate(poses):
            for b, pose in enumerate(pair):
                if pose is None:
                    frames[p, b] = frames[p - 1, b]
                    continue
                pose = np.asarray(pose, dtype=F32)
                assert abs(pose[0]) <= 50 and abs(pose[1]) <= 50
                placed = pose.copy()
                placed[0] += cx; placed[1] += cy
                if p == 0:
                    assert len(pose) == 3
                    start[b] = placed
                frames[p, b] = frame(*placed) if len(pose) == 3 else placed
        static = np.array([min(size_a) == 0, min(size_b) == 0])
        if swap:
            size, static, start, frames = size[::-1].copy(), static[::-1].copy(), start[::-1].copy(), frames[:, ::-1].copy()
        self.cases.append(Case(family, size, static, start, frames))


def _turn(w, h, angle, q):
    """The box of extents (w, h) at `angle`, drawn the same after q quarter turns: ((sx, sy), angle')."""
    a = float(F32(F32(angle) + F32(q) * F32(QUARTER)))
    return ((w, h) if q % 2 == 0 else (h, w)), a


SHIFTS = [1.5, 2.0, 2.5, 3.5]        # along the face: below, on and above ContactPoint::Equals' 2.0, and clear of it
FAR = 40.0


def _face_on_face(b):
    below, above = threshold_angles()
    rel_angles = [0.0, below[-1], above[0], -below[0], -above[-1]]
    n = 0
    for wa, ha, wb, hb in [(4.0, 2.0, 4.0, 2.0), (6.0, 2.0, 2.0, 1.5), (2.0, 1.5, 6.0, 2.0)]:
        offsets = [0.0, min(wa, wb), -min(wa, wb)] + ([wa - wb, wb - wa] if wa != wb else [])
        for dx in offsets:
            for rel in rel_angles:
                for qa in range(4):
                    for qb in range(4):
                        for swap in (False, True):
                            if rel != 0.0 and (qa + qb + swap) % 2:      # the tilted ones at half the turn combinations
                                continue
                            sa, aa = _turn(wa, ha, 0.0, qa)
                            sb, ab = _turn(wb, hb, rel, qb)
                            y = ha + hb - 0.25
                            s = SHIFTS[n % 4] * (1 if (n // 4) % 2 == 0 else -1)
                            later = [(None, None),                                   # kept: merge into the cached slots
                                     (None, (dx + s, y, ab)),                         # B alone along the face
                                     ((s, 0.0, aa), None),                            # A follows: the pose of phase 1, moved as one
                                     (None, (dx + s, y + 0.5, ab)),                   # lifted clear
                                     (None, (dx + s, y + FAR, ab)),                   # far: dead
                                     ((0.0, 0.0, aa), (dx, y, ab))]                   # back after death
                            b.add("face", sa, sb, (0.0, 0.0, aa), (dx, y, ab), later, swap)
                            n += 1


def _threshold_frames(b):
    """A axis-aligned by frame, B's frame with sin exactly 0.1f -3 .. +3 ulps (phase 2 on: phase 1 takes an angle)."""
    n = 0
    for k in range(-3, 4):
        for sign in (1, -1):
            for qb in range(4):
                for dx in (0.0, 3.0, -3.0):
                    for swap in (False, True):
                        s = sign * _ulps(0.1, k)
                        wb, hb = (4.0, 2.0) if qb % 2 == 0 else (2.0, 4.0)
                        y = 2.0 + 2.0 - 0.125
                        fa = np.array([0, 0, 1, 0, 0, 1], dtype=F32)
                        fb = tilted_frame(dx, y, s, qb)
                        shift = SHIFTS[n % 4]
                        fb2 = fb.copy(); fb2[0] += shift
                        later = [(fa, fb), (None, None), (None, fb2), (None, fb)]
                        b.add("threshold", (4.0, 2.0), (wb, hb), (0.0, 0.0, 0.0), (dx, y, sign * 0.1 + qb * QUARTER), later, swap)
                        n += 1


def _vertex_on_face(b):
    n = 0
    for wa, ha in [(6.0, 2.0)]:
        for wb, hb in [(2.0, 2.0), (3.0, 1.0)]:
            for phi in (0.3, 0.7854, 1.2):
                fr = frame(0, 0, phi)
                corners = [(sx * wb * fr[2] + sy * hb * fr[4], sx * wb * fr[3] + sy * hb * fr[5]) for sx in (-1, 1) for sy in (-1, 1)]
                vx, vy = min(corners, key=lambda c: c[1])
                for at in (-wa - 0.5, -wa, -wa + 0.5, -wa / 2, 0.0, wa / 2, wa - 0.5, wa, wa + 0.5):
                    for qa in range(4):
                        for swap in (False, True):
                            sa, aa = _turn(wa, ha, 0.0, qa)
                            x, y = float(at - vx), float(ha - vy - 0.25)
                            s = SHIFTS[n % 4] * (1 if (n // 4) % 2 == 0 else -1)
                            later = [(None, None), (None, (x + s, y, phi)), (None, (x, y, phi)), ((s, 0.0, aa), (x + s, y, phi)),
                                     (None, (x + s, y + 0.5, phi)), (None, (x + s, y + FAR, phi)), ((0.0, 0.0, aa), (x, y, phi))]
                            b.add("vertex", sa, (wb, hb), (0.0, 0.0, aa), (x, y, phi), later, swap)
                            n += 1


def _small_extents(b):
    below, _ = threshold_angles()
    n = 0
    # one small box on a large one
    for s in SMALL:
        for sb in ((s, s), (s, 3.0), (3.0, s)):
            for rel in (0.0, 0.3, below[-1]):
                for dx in (0.0, 2.5, 4.0, 4.5):
                    for swap in (False, True):
                        y = 2.0 + sb[1] - 0.125
                        shift = SHIFTS[n % 4]
                        later = [(None, None), (None, (dx - shift, y, rel)), (None, (dx - shift, y + 0.25, rel)), (None, (dx, y + FAR, rel)),
                                 (None, (dx, y, rel))]
                        b.add("small", (4.0, 2.0), sb, (0.0, 0.0, 0.0), (dx, y, rel), later, swap)
                        n += 1
    # both small
    for s1 in SMALL:
        for s2 in SMALL:
            for sa in ((s1, s1), (s1, 2.0)):
                for sb in ((s2, s2), (2.0, s2)):
                    for config in range(5):
                        for swap in (False, True):
                            rx, ry = sa[0] + sb[0], sa[1] + sb[1]
                            pos, ang = [((0.0, ry - 0.125), 0.0), ((0.0, ry), 0.0), ((rx - 0.125, ry - 0.125), 0.0),
                                        ((0.0, ry - 0.125), 0.7854), ((0.25, ry + 0.0625), 0.05)][config]
                            later = [(None, None), (None, (pos[0] + 0.5, pos[1], ang)), (None, (pos[0] + 0.5, pos[1] + 0.25, ang)),
                                     (None, (pos[0], pos[1] + FAR, ang)), (None, (pos[0], pos[1], ang))]
                            b.add("small2", sa, sb, (0.0, 0.0, 0.0), (pos[0], pos[1], ang), later, swap)
                            n += 1


def _axes_and_depth(b):
    """AABBs overlapping with each SAT axis in turn the first to separate; and a depth of exactly 0 on each axis."""
    big, small = (6.0, 3.0), (3.0, 2.0)
    for swap in (False, True):
        for q in range(4):
            # sep0 / sep1: A tilted, B tucked beside its corner, clear along A's own x or y axis but inside A's AABB
            sa, aa = _turn(big[0], big[1], 0.5, q)
            for along in ("x", "y"):
                fr = frame(0, 0, 0.5)
                ax = (fr[2], fr[3]) if along == "x" else (fr[4], fr[5])
                reach = (big[0] if along == "x" else big[1]) + 1.0 + 0.05
                for side in (1, -1):
                    pos = (float(side * ax[0] * reach), float(side * ax[1] * reach))
                    b.add("axes", sa, (0.7, 0.7), (0.0, 0.0, aa), (pos[0], pos[1], 0.5), [(None, None)], swap)
            # sep2 / sep3: the same with B the tilted one and A small and upright
            sb, ab = _turn(big[0], big[1], 0.5, q)
            for along in ("x", "y"):
                fr = frame(0, 0, 0.5)
                ax = (fr[2], fr[3]) if along == "x" else (fr[4], fr[5])
                reach = (big[0] if along == "x" else big[1]) + 0.9 * (abs(float(ax[0])) + abs(float(ax[1]))) + 0.05
                for side in (1, -1):
                    pos = (float(side * ax[0] * reach), float(side * ax[1] * reach))
                    b.add("axes", (0.9, 0.9), sb, (pos[0], pos[1], 0.0), (0.0, 0.0, ab), [(None, None)], swap)
            # depth exactly 0: integer coordinates, touching along x or y (frames by angle 0 and by exact frame)
            for dx, dy in ((big[0] + small[0], 1.0), (-big[0] - small[0], -1.0), (1.0, big[1] + small[1]), (-1.0, -big[1] - small[1])):
                exact_a = np.array([0, 0, 1, 0, 0, 1], dtype=F32)
                exact_b = np.array([dx, dy, 1, 0, 0, 1], dtype=F32)
                if q % 2:
                    exact_b = np.array([dx, dy, -1, 0, 0, -1], dtype=F32)
                b.add("depth0", big, small, (0.0, 0.0, 0.0), (dx, dy, 0.0), [(exact_a, exact_b), (None, None), (None, (dx, dy, 0.0))], swap)


def _two_new_points_close(b):
    """Two cached points, then a pose whose two new points lie within 2 of each other and of neither cached one: the second merges
    into the slot the first has just appended (merge_slot2)."""
    n = 0
    for w in (1.25, 1.5, 1.75, 1.9):
        for big in (6.0, 8.0):
            for jump in (4.0, -4.0, 5.5):
                for swap in (False, True):
                    # phase 1: the narrow box B (half-width w < 2: its two contacts lie 2w < 4 apart, more than 2: both kept) ...
                    y = 2.0 + 1.5 - 0.125
                    later = [(None, None), (None, (jump, y, 0.0)), (None, (jump + 1.0, y, 0.0)), (None, (0.0, y + 0.5, 0.0)), (None, (0.0, y, 0.0))]
                    b.add("close", (big, 2.0), (w, 1.5), (0.0, 0.0, 0.0), (0.0, y, 0.0), later, swap)
                    # ... and a half-width of 1 or less collapses the edge; just above, the two points are 2 apart or closer
                    b.add("close", (big, 2.0), (1.0 + (w - 1.25) / 16, 1.5), (0.0, 0.0, 0.0), (0.0, y, 0.0), later, swap)
                    n += 1


def _lying_then_upright(b):
    """Two cached points under a box lying on its long side, then the box upright somewhere else: its two new points equal neither
    cached one and lie 2w apart.  w = 1: exactly 2, so the second merges into the slot the first has just appended (merge_slot2);
    w > 1: the second is appended too (append_slot3)."""
    for w in (1.0, 1.125, 1.25):
        for jump in (6.5, -6.5, 6.625):         # (more than 2 beyond the cached points at +-3 on the lower box)
            for qa in (0, 2):
                for swap in (False, True):
                    sa, aa = _turn(8.0, 2.0, 0.0, qa)
                    lying, upright = (0.0, 2.0 + w - 0.125, QUARTER), (jump, 2.0 + 3.0 - 0.125, 0.0)
                    later = [(None, None), (None, upright), (None, None), (None, lying), (None, upright)]
                    b.add("upright", sa, (w, 3.0), (0.0, 0.0, aa), lying, later, swap)


def _plates(b):
    """A plate without thickness, tilted a little, crossing a box's face near its end: both of the plate's faces are the same
    segment, so the edge-edge candidates pair up in the ways two solid boxes give only on a knife's edge (ee_pick03, ee_pick12)."""
    for h in (0.25, 2.0):
        for w in (3.0, 4.25):
            for tilt in (0.05, -0.05, 0.0674, -0.0674):
                for half_turn in (0.0, 2 * QUARTER):
                    for side in (1.0, -1.0):
                        for lift in (0.125, 0.375):
                            for swap in (False, True):
                                x = side * (8.0 - w + 2.5)
                                pose = (x, h + lift, tilt + half_turn)
                                later = [(None, None), (None, (x - side * 2.0, h + lift, tilt + half_turn)), (None, pose)]
                                b.add("plate", (8.0, h), (w, 0.0), (0.0, 0.0, 0.0), pose, later, swap)


def _random(b, count, seed):
    rng = np.random.default_rng(seed)
    sizes = np.array(SMALL + [1.5, 2.0, 3.0, 5.0, 8.0, 12.0])
    angles = np.array([0.0, 0.05, 0.0995, 0.1002, 0.1005, 0.3, 0.7854, 1.4706, 1.5708, 3.1416, -1.5708, -0.1002])
    for i in range(count):
        def size():
            v = [float(rng.choice(sizes)) if rng.random() < 0.5 else float(rng.uniform(0, 12)) for _ in range(2)]
            return (v[0], v[1])
        def angle():
            return float(rng.choice(angles) + rng.choice([0.0, QUARTER, 2 * QUARTER, -QUARTER])) if rng.random() < 0.6 else float(rng.uniform(-3.2, 3.2))
        sa, sb, aa, ab = size(), size(), angle(), angle()
        rx, ry = sa[0] + sb[0], sa[1] + sb[1]
        slack = 0.0 if rng.random() < 0.3 else float(rng.normal(0, 0.6))
        along, sign = float(rng.uniform(-1.1, 1.1)), float(rng.choice([-1.0, 1.0]))
        if rng.random() < 0.5:
            pos = (sign * (rx + slack), along * ry)
        else:
            pos = (along * rx, sign * (ry + slack))
        pos = (float(np.clip(pos[0], -26, 26)), float(np.clip(pos[1], -26, 26)))
        arrive = int(rng.integers(0, 3))                  # the phase in which the pair first comes together (0: at once)
        poses = []
        a_pose, b_pose = (0.0, 0.0, aa), (pos[0], pos[1], ab)
        for p in range(MAX_PHASES - arrive):
            if p:
                kind = int(rng.integers(0, 7))
                step = float(rng.choice([0.5, 1.9, 2.0, 2.1, 3.0, -2.0, -2.1, 6.0]))
                if kind == 1:
                    b_pose = (b_pose[0] + step, b_pose[1], b_pose[2])
                elif kind == 2:
                    b_pose = (b_pose[0], b_pose[1] + step, b_pose[2])
                elif kind == 3:
                    b_pose = (b_pose[0], b_pose[1], b_pose[2] + float(rng.choice([0.01, -0.01, 0.1, QUARTER])))
                elif kind == 4:
                    a_pose = (a_pose[0] + step, a_pose[1], a_pose[2]); b_pose = (b_pose[0] + step, b_pose[1], b_pose[2])
                elif kind == 5:
                    a_pose = (a_pose[0], a_pose[1] + step, a_pose[2])
                b_pose = (float(np.clip(b_pose[0], -49, 49)), float(np.clip(b_pose[1], -49, 49)), b_pose[2])
                a_pose = (float(np.clip(a_pose[0], -20, 20)), float(np.clip(a_pose[1], -20, 20)), a_pose[2])
            poses.append((a_pose, b_pose))
        away = [((0.0, -24.0, aa), (pos[0], 24.0 + 12.0, ab))] * arrive
        poses = away + poses
        b.add("random", sa, sb, poses[0][0], poses[0][1], poses[1:], bool(rng.random() < 0.5))


_cases = None


def cases():
    """The corpus, in case order (built once)."""
    global _cases
    if _cases is None:
        b = _Builder()
        _lying_then_upright(b)                # (the first 129 cases and more have positive half-extents: worlds of them build by add_scene)
        _two_new_points_close(b)
        _axes_and_depth(b)
        _plates(b)
        _threshold_frames(b)
        _vertex_on_face(b)
        _small_extents(b)
        _face_on_face(b)
        _random(b, 1500, 20260)
        _cases = b.cases
    return _cases


def scene(cs):
    """The add_scene dictionary of phase 1: case k's boxes are bodies 2k and 2k + 1."""
    start = np.concatenate([c.start for c in cs])
    size = np.concatenate([c.size for c in cs])
    return {"px": start[:, 0].copy(), "py": start[:, 1].copy(), "angle": start[:, 2].copy(), "sx": size[:, 0].copy(), "sy": size[:, 1].copy(),
            "static": np.concatenate([c.static for c in cs])}


def phase_frames(cs, phase):
    """(2 * len(cs), 6) float32: every body's frame in `phase` (0-based); a case past its last phase keeps its last pose."""
    return np.concatenate([c.frames[min(phase, len(c.frames) - 1)] for c in cs])
