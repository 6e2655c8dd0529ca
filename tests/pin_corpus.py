"""Directed pins: small worlds the chains and pairs of tests/test_pins_gpu.py never build, each named for what it reaches
(tests/test_pin_corpus_cpu.py proves the claims on the CPU with the host-only schedule builder and pin_spec.prestep and holds the
spec to the float64 reference, tests/pin_reference.py; tests/test_pin_corpus_gpu.py runs every motif on the device).

A motif is a Motif below: body rows (px, py, angle, half x, half y, static) with NON-ZERO initial angles, inverse masses where they
are not AddBody's, initial velocities (every dynamic body has one, seeded by the motif's name; a static body only where the motif
is about that), the pins with the impulse they are added with, and the claims:
  flags     per pin (active, write_a, write_b) as pin_spec.prestep must find them on the initial state
  shape     (classes, sizes of the groups, LDS groups) of the pin schedule at the default cap of 256 (or at `cap`)
  k12_zero  pins whose k12 is exactly 0
  noise_det the (one) pin's K is singular and its float32 det expression is positive all the same: what the floor of the activity rule is for
Bodies that no pin joins are far enough apart, and the joined ones short enough of their pins' points, that no two boxes'
AABBs meet in the steps a test runs: the manifold count stays 0, so the velocities after a step are the pin pass's output.

MULTI are the motifs with more than one pin: the GPU file runs them a second time under PHX_PIN_GROUP_PINS=1, where a connected
component of two pins or more exceeds the cap and goes to the trailing group (k_pin_prestep / k_pin_class) whole.

Measured, per motif: the spec's deviation from the float64 reference as a multiple of the reference's own float32-vs-float64
deviation (`noise`, floored at one float32 ulp, 1.19e-07), in the metric of pin_reference.deviation; the worst of the sweep counts
run (1, 8, and 64 on triangle and hub5) with its figures.  The bound is 8.  The device's velocities are the spec's byte for byte on
both paths, so its ratios are these.  No motif's noise is above 1e-3: none is excluded from the comparison (lever100 stays in, at
1.5e-05; the singular motifs are inactive on both sides and compare at 0).
  motif                         noise       spec   ratio
  pair                       5.67e-07   6.18e-07    1.09   (n = 1)
  b1_static                  5.78e-07   8.69e-07    1.50   (n = 1)
  static_static              1.19e-07          0    0.00   (n = 8)
  static_world               1.19e-07          0    0.00   (n = 8)
  kinematic_anchor           1.41e-06   1.41e-06    1.00   (n = 8)
  no_rotation                2.23e-06   2.23e-06    1.00   (n = 8)
  centres                    1.19e-07   9.93e-09    0.08   (n = 8)
  lever100                   1.48e-05    5.1e-05    3.44   (n = 1)
  warm                       3.84e-06   4.46e-06    1.16   (n = 1)
  triangle                   9.91e-06   1.02e-05    1.03   (n = 1)
  ring5                      2.18e-06   2.48e-06    1.14   (n = 1)
  ring6_cap4                 3.77e-06   3.83e-06    1.02   (n = 1)
  double_pin                 5.19e-06   5.26e-06    1.01   (n = 8)
  double_pin_swapped         2.93e-06    3.1e-06    1.06   (n = 1)
  grid8x8                    1.19e-05    1.2e-05    1.00   (n = 1)
  hub5                       4.66e-06    4.7e-06    1.01   (n = 8)
  hub63                      1.13e-05   1.14e-05    1.00   (n = 1)
  hub64                      9.37e-06   9.37e-06    1.00   (n = 1)
  hub65                      1.63e-05   1.63e-05    1.00   (n = 8)
  hub130                     2.22e-05   2.22e-05    1.00   (n = 8)
  static_hub300              2.48e-05   2.47e-05    1.00   (n = 8)
  own_statics256             3.96e-05   3.98e-05    1.00   (n = 1)
  chain256                    8.3e-05    8.3e-05    1.00   (n = 8)
  chain257                   8.06e-05   8.06e-05    1.00   (n = 8)
  inactive_beside_active     2.06e-06   2.12e-06    1.03   (n = 1)
  axle_world                 1.19e-07          0    0.00   (n = 8)
  axle_centre                1.19e-07          0    0.00   (n = 8)
  axles_in_line              1.19e-07          0    0.00   (n = 8)
  axle_dynamic               1.23e-06   1.55e-06    1.26   (n = 1)
  200 random 6-chains          5.43e-07   6.36e-07    1.17   (n = 1; n = 8: 1.00; the worst single chain 3.44)
"""
import zlib

import numpy as np

from phyx_amd.api import pin_dtype
import pin_reference as ref

DT = 1.0 / 60.0
G = -200.0
EXCLUDE_ABOVE = 1e-3                                     # a float32-vs-float64 deviation above this: no float64 comparison
MAY_BE_EXCLUDED = ("lever100", "axle_world", "axle_centre", "axles_in_line")
ON = (True, True, True)


class Motif:
    def __init__(self, name):
        self.name = name
        self.rows, self.masses, self.vel = [], {}, {}
        self._pins, self.flags, self.k12_zero = [], [], []
        self.shape, self.cap, self.steps, self.gravity = None, None, 5, G
        self.iterations = (8,)
        self.noise_det = False                                  # K is singular and the float32 det expression comes out positive
        self._rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)

    # ---- building ----
    def body(self, x, y, half=(3.0, 1.0), angle=None, static=False, mass=None, vel=None):
        i = len(self.rows)
        if angle is None:
            angle = 0.3 + 0.7 * ((i * 0.618034) % 1.0)              # never 0, never the same twice in a row
        self.rows.append((float(x), float(y), float(angle), float(half[0]), float(half[1]), bool(static)))
        if mass is not None:
            self.masses[i] = (float(mass[0]), float(mass[1]))
        if vel is None and not static:
            v = self._rng.uniform(-3.0, 3.0, 2)
            vel = (v[0], v[1], self._rng.uniform(-0.3, 0.3))
        if vel is not None:
            self.vel[i] = tuple(float(c) for c in vel)
        return i

    def local(self, i, point):
        """the world point in body i's frame"""
        x, y, a = self.rows[i][:3]
        c, s, dx, dy = np.cos(a), np.sin(a), point[0] - x, point[1] - y
        return (c * dx + s * dy, -s * dx + c * dy)

    def pin(self, a, b, anchor1, anchor2, flags=ON, impulse=(0.0, 0.0)):
        self._pins.append((a, b, anchor1, anchor2, impulse))
        self.flags.append(tuple(bool(f) for f in flags))
        return len(self._pins) - 1

    def pin_at(self, a, b, point, flags=ON, impulse=(0.0, 0.0), slack=(0.0, 0.0)):
        """a pin of a and b (-1: the world) whose anchors both lie at the world point `point`, body2's `slack` away from it"""
        other = (point[0] + slack[0], point[1] + slack[1])
        return self.pin(a, b, self.local(a, point), other if b < 0 else self.local(b, other), flags, impulse)

    # ---- reading ----
    @property
    def pins(self):
        p = np.zeros(len(self._pins), dtype=pin_dtype)
        for k, row in enumerate(self._pins):
            p[k] = row
        return p

    def scene(self):
        r = np.asarray([row[:5] for row in self.rows], dtype=np.float32).reshape(-1, 5)
        return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": r[:, 2].copy(), "sx": r[:, 3].copy(), "sy": r[:, 4].copy(),
                "static": np.asarray([row[5] for row in self.rows], dtype=bool)}

    def is_static(self):
        st = [row[5] for row in self.rows]
        for i, m in self.masses.items():
            st[i] = m == (0.0, 0.0)
        return np.asarray(st, dtype=np.uint8)

    def graph(self):
        p = self.pins
        return p["body1"].tolist(), p["body2"].tolist(), self.is_static().tolist()

    def oracle_world(self, binding, gravity=None):
        """the oracle World of the motif with its masses and velocities set"""
        w = binding.OracleWorld(self.gravity if gravity is None else gravity)
        w.add_scene(self.scene())
        b = w.bodies()
        for i, (m, ii) in self.masses.items():
            b["inv_mass"][i], b["inv_inertia"][i] = m, ii
        for i, v in self.vel.items():
            b["velocity"]["x"][i], b["velocity"]["y"][i], b["angular_velocity"][i] = v
        return w

    def device_world(self, phyx_amd, gravity=None):
        """the device World of the motif with its masses, velocities and pins"""
        w = phyx_amd.World(0, gravity=self.gravity if gravity is None else gravity)
        w.add_scene(self.scene())
        if self.masses:
            idx = sorted(self.masses)
            w.set_inverse_masses(np.asarray(idx, dtype=np.int32), np.asarray([self.masses[i] for i in idx], dtype=np.float32))
        if self.vel:
            idx = sorted(self.vel)
            w.set_velocities(np.asarray(idx, dtype=np.int32), np.asarray([self.vel[i] for i in idx], dtype=np.float32))
        got = w.add_pins(self.pins)
        assert got.tolist() == list(range(len(self._pins)))
        return w


def check_schedule(body1, body2, is_static, s, cap, name=""):
    """What every pin schedule must satisfy: each pin once, the offsets well formed, no class spanning two groups, at most one trailing
    group, no LDS group above the cap, no dynamic body twice in a class, no dynamic body in two groups."""
    n = len(body1)
    order, coff, goff = s["order"], s["class_offsets"], s["group_offsets"]
    assert sorted(order.tolist()) == list(range(n)), "every pin appears once"
    assert coff[0] == 0 and coff[-1] == n and goff[0] == 0 and goff[-1] == n
    assert (np.diff(coff) > 0).all() and (np.diff(goff) > 0).all()
    assert set(goff.tolist()) <= set(coff.tolist()), "a class never spans two groups"
    assert 0 <= s["lds_groups"] <= len(goff) - 1 and len(goff) - 1 - s["lds_groups"] <= 1, "at most one trailing group"

    def dynamic(k):
        return {b for b in (body1[k], body2[k]) if b >= 0 and not is_static[b]}

    for c in range(len(coff) - 1):                      # the classes share no dynamic body
        seen = set()
        for k in order[coff[c]:coff[c + 1]]:
            d = dynamic(int(k))
            assert not (seen & d), "class %d of %s shares a dynamic body" % (c, name)
            seen |= d
    owner = {}
    for g in range(len(goff) - 1):                      # the groups are body-disjoint, statics and the world aside
        assert goff[g + 1] - goff[g] <= cap or g >= s["lds_groups"], "an LDS group exceeds the cap"
        for k in order[goff[g]:goff[g + 1]]:
            for b in dynamic(int(k)):
                assert owner.setdefault(b, g) == g, "body %d is in two groups" % b


def shape_of(s):
    """(classes, group sizes, LDS groups) of a schedule"""
    return len(s["class_offsets"]) - 1, np.diff(s["group_offsets"]).tolist(), int(s["lds_groups"])


# ---- the motifs ----
MOTIFS = {}


def motif(fn):
    MOTIFS[fn.__name__] = fn
    return fn


def build(name):
    m = Motif(name)
    MOTIFS[name](m)
    assert m.shape is not None and len(m.flags) == len(m._pins)
    return m


def _ring_points(count, first_radius=14.0, spacing=8.0, step=8.0):
    """`count` points on rings around the origin, `spacing` apart along a ring, the rings `step` apart"""
    out, r = [], first_radius
    while len(out) < count:
        k = int(2.0 * np.pi * r / spacing)
        out += [(r * np.cos(2.0 * np.pi * j / k + 0.1), r * np.sin(2.0 * np.pi * j / k + 0.1)) for j in range(k)]
        r += step
    return out[:count]


def _hub(m, degree, static=False, hub_is_body1=False):
    hub = m.body(0.0, 0.0, half=(4.0, 4.0), static=static, vel=None if static else (1.0, -0.5, 0.05))
    for x, y in _ring_points(degree):
        r = np.hypot(x, y)
        s = m.body(x, y, half=(1.5, 1.0))
        at = (x - 2.0 * x / r, y - 2.0 * y / r)                      # short of the spoke, on the hub's side
        if hub_is_body1:
            m.pin_at(hub, s, at, flags=(True, not static, True))
        else:
            m.pin_at(s, hub, at, flags=(True, True, not static))


# -- flags and ends --
@motif
def pair(m):
    """two dynamic bodies, one pin, no impulse: the block solve that one sweep must leave exact"""
    a, b = m.body(0.0, 0.0), m.body(10.0, 0.0, half=(4.0, 1.5))
    m.pin_at(a, b, (5.0, 0.5), slack=(0.2, -0.1))
    m.shape = (1, [1], 1)
    m.iterations = (8, 1)


@motif
def b1_static(m):
    """body1 static, body2 dynamic: write_a false beside a written body2"""
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    b = m.body(12.0, 0.0)
    m.pin_at(a, b, (8.0, 1.0), flags=(True, False, True), slack=(0.1, -0.05))
    m.shape = (1, [1], 1)
    m.iterations = (8, 1)


@motif
def static_static(m):
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    b = m.body(30.0, 0.0, half=(5.0, 5.0), static=True)
    m.pin_at(a, b, (15.0, 0.0), flags=(False, False, False), impulse=(7.0, -7.0))
    m.shape = (1, [1], 0)


@motif
def static_world(m):
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    m.pin_at(a, -1, (8.0, 0.0), flags=(False, False, False), impulse=(1.0, 2.0), slack=(0.5, 0.5))
    m.shape = (1, [1], 0)


@motif
def kinematic_anchor(m):
    """a static body with a linear and an angular velocity: IntegratePosition moves it, and what hangs on it follows; one pin has it
    as body2 and one as body1"""
    k = m.body(0.0, 0.0, half=(5.0, 2.0), static=True, vel=(6.0, 3.0, 0.8))
    a = m.body(12.0, 0.0)
    b = m.body(-12.0, 0.0)
    m.pin_at(a, k, (8.0, 0.5), flags=(True, True, False))
    m.pin_at(k, b, (-8.0, -0.5), flags=(True, False, True))
    m.shape = (1, [2], 1)


@motif
def no_rotation(m):
    """inv_mass > 0 with inv_inertia == 0: a body that moves and cannot turn"""
    a = m.body(0.0, 0.0, mass=(500.0, 0.0), vel=(2.0, -1.0, 0.4))
    b = m.body(10.0, 0.0)
    m.pin_at(a, b, (5.0, 0.5))
    m.pin_at(a, -1, (-5.0, 0.0), flags=(True, True, False))
    m.shape = (2, [2], 1)


@motif
def centres(m):
    """anchors at both centres: no lever arm, k12 == 0; the bodies start 12 apart, so the bias pulls hard"""
    a = m.body(0.0, 0.0, half=(0.5, 0.5))
    b = m.body(12.0, 0.0, half=(0.5, 0.5))
    c = m.body(0.0, 30.0, half=(0.5, 0.5))
    m.k12_zero = [m.pin(a, b, (0.0, 0.0), (0.0, 0.0)), m.pin(c, -1, (0.0, 0.0), (1.0, 31.0), flags=(True, True, False))]
    m.shape = (1, [2], 1)
    m.steps = 4


@motif
def lever100(m):
    """a lever arm of 100: i r^2 is a thousand times the inverse mass"""
    a = m.body(0.0, 0.0, angle=0.4)
    m.pin(a, -1, (100.0, 0.0), (100.0 * np.cos(0.4), 100.0 * np.sin(0.4)), flags=(True, True, False))
    m.shape = (1, [1], 1)
    m.iterations = (8, 1)


@motif
def warm(m):
    """pins added with a non-zero impulse: the warm start of the first step applies it"""
    a, b, c = m.body(0.0, 0.0), m.body(10.0, 0.0), m.body(20.0, 0.0)
    m.pin_at(a, -1, (-5.0, 0.0), flags=(True, True, False), impulse=(2e-4, -3e-4))
    m.pin_at(b, a, (5.0, 0.0), impulse=(-1e-4, 4e-4))
    m.pin_at(c, b, (15.0, 0.0), impulse=(3e-4, 1e-4))
    m.shape = (2, [3], 1)


# -- topology --
@motif
def triangle(m):
    pts = [(0.0, 0.0), (12.0, 0.0), (6.0, 10.0)]
    ids = [m.body(x, y, half=(2.0, 1.0)) for x, y in pts]
    for k in range(3):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % 3]
        m.pin_at(ids[k], ids[(k + 1) % 3], ((x0 + x1) / 2, (y0 + y1) / 2))
    m.shape = (3, [3], 1)
    m.iterations = (8, 1, 64)


@motif
def ring5(m):
    pts = [(12.0 * np.cos(2 * np.pi * k / 5), 12.0 * np.sin(2 * np.pi * k / 5)) for k in range(5)]
    ids = [m.body(x, y, half=(2.0, 1.0)) for x, y in pts]
    for k in range(5):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % 5]
        m.pin_at(ids[(k + 1) % 5] if k % 2 else ids[k], ids[k] if k % 2 else ids[(k + 1) % 5], ((x0 + x1) / 2, (y0 + y1) / 2))
    m.shape = (3, [5], 1)


@motif
def ring6_cap4(m):
    """a cycle that exceeds the cap: the trailing group at an even cycle's two classes"""
    pts = [(14.0 * np.cos(2 * np.pi * k / 6), 14.0 * np.sin(2 * np.pi * k / 6)) for k in range(6)]
    ids = [m.body(x, y, half=(2.0, 1.0)) for x, y in pts]
    for k in range(6):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % 6]
        m.pin_at(ids[k], ids[(k + 1) % 6], ((x0 + x1) / 2, (y0 + y1) / 2))
    m.shape, m.cap = (2, [6], 0), 4


@motif
def double_pin(m):
    """two pins on one pair, the same ends: together they lock the pair"""
    a, b = m.body(0.0, 0.0), m.body(10.0, 0.0)
    m.pin_at(a, b, (5.0, 2.0))
    m.pin_at(a, b, (5.0, -2.0))
    m.shape = (2, [2], 1)


@motif
def double_pin_swapped(m):
    a, b = m.body(0.0, 0.0), m.body(10.0, 0.0)
    m.pin_at(a, b, (5.0, 2.0))
    m.pin_at(b, a, (5.0, -2.0))
    m.shape = (2, [2], 1)


@motif
def grid8x8(m):
    ids = [[m.body(12.0 * i, 12.0 * j, half=(2.0, 2.0)) for i in range(8)] for j in range(8)]
    for j in range(8):
        for i in range(8):
            if i < 7:
                m.pin_at(ids[j][i], ids[j][i + 1], (12.0 * i + 6.0, 12.0 * j))
            if j < 7:
                m.pin_at(ids[j + 1][i], ids[j][i], (12.0 * i, 12.0 * j + 6.0))
    m.shape = (5, [112], 1)


@motif
def hub5(m):
    _hub(m, 5)
    m.shape = (5, [5], 1)
    m.iterations = (8, 1, 64)


@motif
def hub63(m):
    _hub(m, 63)
    m.shape = (63, [63], 1)


@motif
def hub64(m):
    _hub(m, 64, hub_is_body1=True)
    m.shape = (64, [64], 1)


@motif
def hub65(m):
    """past 64 colours the colouring widens its masks and starts over; more classes than an LDS group takes: the trailing group"""
    _hub(m, 65)
    m.shape = (65, [65], 0)


@motif
def hub130(m):
    _hub(m, 130, hub_is_body1=True)
    m.shape = (130, [130], 0)
    m.steps = 3


@motif
def static_hub300(m):
    """a static body shared by five LDS groups"""
    _hub(m, 300, static=True)
    m.shape = (5, [64, 64, 64, 64, 44], 5)
    m.steps = 4


@motif
def own_statics256(m):
    """256 pins, each dynamic body on a static body of its own"""
    for k in range(256):
        x, y = 24.0 * (k % 16), 16.0 * (k // 16)
        s = m.body(x, y, half=(2.0, 2.0), static=True)
        d = m.body(x + 9.0, y)
        if k % 2:
            m.pin_at(s, d, (x + 5.0, y + 0.5), flags=(True, False, True))
        else:
            m.pin_at(d, s, (x + 5.0, y + 0.5), flags=(True, True, False))
    m.shape = (4, [64, 64, 64, 64], 4)
    m.steps = 4


def _chain(m, links, tilt=0.4, spacing=10.0, row=30):
    """a chain from the world laid in rows of `row` links joined by one link across, the whole turned by `tilt` about the origin: folded
    so that it stays near the origin (a straight chain of 256 reaches x = 2560, where float32 positions resolve 2.4e-4 and the
    separation C, a difference of positions, has lost its digits before the pass begins)"""
    joints, x, y, step = [(0.0, 0.0)], 0.0, 0.0, 1.0
    while len(joints) <= links:
        for _ in range(row):
            x += step * spacing
            joints.append((x, y))
        y += spacing
        joints.append((x, y))
        step = -step
    joints = np.asarray(joints[:links + 1]) - np.array([row * spacing / 2.0, spacing * (links // (row + 1)) / 2.0])
    c, s = np.cos(tilt), np.sin(tilt)
    joints = joints @ np.array([[c, s], [-s, c]])
    h = spacing / 2.0
    for k in range(links):
        d = joints[k + 1] - joints[k]
        mid = (joints[k] + joints[k + 1]) / 2.0
        body = m.body(mid[0], mid[1], half=(2.5, 0.8), angle=float(np.arctan2(d[1], d[0])))
        if k == 0:
            m.pin(body, -1, (-h, 0.0), (float(joints[0][0]), float(joints[0][1])), flags=(True, True, False))
        else:
            m.pin(body, body - 1, (-h, 0.0), (h, 0.0))


@motif
def chain256(m):
    """exactly the cap: one LDS group of 256 lanes"""
    _chain(m, 256)
    m.shape = (2, [256], 1)
    m.steps = 4


@motif
def chain257(m):
    """one past the cap: the trailing group"""
    _chain(m, 257)
    m.shape = (2, [257], 0)
    m.steps = 4


@motif
def inactive_beside_active(m):
    """a pin between static bodies beside a dynamic pair: an LDS group and a trailing group of inactive pins in one schedule"""
    a = m.body(0.0, 0.0, half=(5.0, 5.0), static=True)
    b = m.body(30.0, 0.0, half=(5.0, 5.0), static=True)
    c, d = m.body(0.0, 40.0), m.body(10.0, 40.0)
    m.pin_at(a, b, (15.0, 0.0), flags=(False, False, False), impulse=(3.0, 4.0))
    m.pin_at(c, d, (5.0, 40.5))
    m.shape = (2, [1, 1], 1)


# -- the singular pin --
def _axle_mass(half=(3.0, 1.0)):
    from phyx_amd.api import pinned_inv_inertia
    return (0.0, pinned_inv_inertia(*half))


@motif
def axle_world(m):
    """a wheel on a fixed axle (inv_mass 0, inv_inertia > 0) pinned off-centre to the world: K is singular, and at this anchor the
    float32 det expression returns +0.5 of 6.25e6: `det > 0` takes it for a determinant"""
    a = m.body(0.0, 0.0, mass=_axle_mass(), vel=(3.0, 0.0, 0.7))
    m.pin_at(a, -1, (2.5, 0.3), flags=(False, True, False), impulse=(1.0, -1.0), slack=(0.3, 0.1))
    m.shape = (1, [1], 1)
    m.noise_det = True


@motif
def axle_centre(m):
    """the wheel pinned at its own centre: K = 0"""
    a = m.body(0.0, 0.0, mass=_axle_mass(), vel=(3.0, 0.0, 0.7))
    m.pin(a, -1, (0.0, 0.0), (0.2, 0.1), flags=(False, True, False), impulse=(1.0, -1.0))
    m.shape = (1, [1], 1)


@motif
def axles_in_line(m):
    """two wheels pinned to each other on the line through their axles: the lever arms are parallel, K is singular; the float32 det
    expression returns +1536 of 6.9e9"""
    a = m.body(0.0, 0.0, mass=_axle_mass(), vel=(0.0, 0.0, 0.7))
    b = m.body(10.0, 5.0, mass=_axle_mass(), vel=(0.0, 0.0, -0.4))
    m.pin_at(a, b, (5.0, 2.5), flags=(False, True, True), impulse=(1.0, -1.0))
    m.shape = (1, [1], 1)
    m.noise_det = True


@motif
def axle_dynamic(m):
    """the wheel pinned to a dynamic body: K is regular, the pin is active and the wheel turns"""
    a = m.body(0.0, 0.0, mass=_axle_mass(), vel=(0.0, 0.0, 0.7))
    b = m.body(10.0, 0.0)
    m.pin_at(a, b, (5.0, 0.5))
    m.pin_at(b, a, (5.0, -0.5))
    m.shape = (2, [2], 1)


NAMES = tuple(MOTIFS)
SINGULAR = ("axle_world", "axle_centre", "axles_in_line")


def _components(m):
    """the number of pins in the largest connected component of the motif's pins (static bodies and the world do not connect)"""
    b1, b2, st = m.graph()
    parent = list(range(len(st)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(b1, b2):
        if b >= 0 and not st[a] and not st[b]:
            parent[find(a)] = find(b)
    size = {}
    for a, b in zip(b1, b2):
        roots = {find(x) for x in (a, b) if x >= 0 and not st[x]}
        for r in roots:
            size[r] = size.get(r, 0) + 1
    return max(size.values(), default=1)


MULTI = tuple(n for n in NAMES if len(build(n)._pins) > 1)
CONNECTED = tuple(n for n in MULTI if _components(build(n)) == len(build(n)._pins))      # under a cap of 1: one trailing group


# ---- the random worlds of the CPU file ----
def random_chain(seed, links=6):
    """a chain of `links` boxes hung from the world, every frame rotated, random anchors, velocities and impulses -> Motif"""
    m = Motif("random_chain_%d" % seed)
    r = m._rng
    for k in range(links):
        m.body(20.0 * k + r.uniform(-2, 2), r.uniform(-5, 5), half=(r.uniform(1.5, 4.0), r.uniform(1.0, 2.5)), angle=r.uniform(-3.1, 3.1),
               vel=(r.uniform(-5, 5), r.uniform(-5, 5), r.uniform(-2, 2)))
    m.pin(0, -1, tuple(r.uniform(-4, 4, 2)), tuple(r.uniform(-4, 4, 2)), flags=(True, True, False))
    for k in range(1, links):
        m.pin(k, k - 1, tuple(r.uniform(-4, 4, 2)), tuple(r.uniform(-4, 4, 2)))
    m.shape = (2, [links], 1)
    return m


def random_axle(seed):
    """the issue's trial: one wheel on a fixed axle with velocity (3, 0), a random frame and a random off-centre world pin"""
    m = Motif("random_axle_%d" % seed)
    r = m._rng
    half = (r.uniform(1.0, 5.0), r.uniform(1.0, 5.0))
    m.body(r.uniform(-50, 50), r.uniform(-50, 50), half=half, angle=r.uniform(-3.1, 3.1), mass=_axle_mass(half), vel=(3.0, 0.0, r.uniform(-2, 2)))
    a1 = r.uniform(-5, 5, 2)
    m.pin(0, -1, tuple(a1), tuple(r.uniform(-50, 50, 2)), flags=(False, True, False), impulse=tuple(r.uniform(-1, 1, 2)))
    m.shape = (1, [1], 1)
    return m


def random_axle_pair(seed):
    """two wheels on fixed axles pinned at a random point of the line through the axles"""
    m = Motif("random_axle_pair_%d" % seed)
    r = m._rng
    pa, pb = r.uniform(-50, 50, 2), r.uniform(-50, 50, 2)
    for p in (pa, pb):
        half = (r.uniform(1.0, 5.0), r.uniform(1.0, 5.0))
        m.body(p[0], p[1], half=half, angle=r.uniform(-3.1, 3.1), mass=_axle_mass(half), vel=(0.0, 0.0, r.uniform(-2, 2)))
    t = r.uniform(-1.0, 2.0)
    m.pin_at(0, 1, tuple(pa + t * (pb - pa)), flags=(False, True, True), impulse=tuple(r.uniform(-1, 1, 2)))
    m.shape = (1, [1], 1)
    return m


# ---- the checks that tests/test_pin_corpus_cpu.py makes on the spec's output and tests/test_pin_corpus_gpu.py on the device's ----
ULP = 2.0 ** -23
U = 2.0 ** -24                  # one float32 rounding
MARGIN = 8.0                    # x the reference's own float32-vs-float64 deviation: the bound of a comparison with the reference


def check_the_anchor_is_followed(m, start, bodies, steps):
    """kinematic_anchor: IntegratePosition moved the static body by its velocities, and the bodies pinned to it went along: their
    pins' separations stay a tenth of the way the pins' points on the anchor travelled (a pin that ignored the anchor's velocity
    would fall behind by all of it)."""
    vx, vy, w = m.vel[0]
    assert abs(float(bodies["pos"]["x"][0]) - float(start["pos"]["x"][0]) - vx * DT * steps) < 1e-4
    assert abs(float(bodies["pos"]["y"][0]) - float(start["pos"]["y"][0]) - vy * DT * steps) < 1e-4
    assert bodies["xv"]["x"][0] != start["xv"]["x"][0], "the anchor never turned"
    st0, st1 = ref.State(start), ref.State(bodies)
    pins = m.pins
    for k in range(len(pins)):
        end = 1 if pins["body1"][k] == 0 else 2
        a = np.asarray(pins["anchor%d" % end][k], dtype=np.float64)
        travelled = np.hypot(*((st1.pos[0] + st1.rot[0] @ a) - (st0.pos[0] + st0.rot[0] @ a)))
        apart = np.hypot(*ref._constraint(st1, pins[k])[5])
        print("pin %d: its point on the anchor travelled %.4g, the pin is %.4g apart" % (k, travelled, apart))
        assert travelled > 0.3 and apart < 0.1 * travelled


ONE_PIN = ("pair", "b1_static", "lever100")


def check_residual(before, after, pin):
    """A block solve is exact up to the rounding of its own arithmetic: cond(K) times a few roundings (16: the spec's sweep is
    about that many operations deep) of the terms the residual is made of, before and after."""
    start, k, terms0 = ref.residual(before, before, pin, DT)
    res, _, terms1 = ref.residual(before, after, pin, DT)
    tol = 16 * U * np.linalg.cond(k) * (terms0 + terms1)
    print("residual %s (before the sweep %s), tolerance %.3g" % (res, start, tol))
    assert np.abs(start).max() > 100 * tol, "the pin had nothing to solve"
    assert np.abs(res).max() <= tol


def conserves_momentum(m):
    b1, b2, st = m.graph()
    return not any(st) and min(b2) >= 0 and not m.masses


CONSERVING = tuple(n for n in NAMES if conserves_momentum(build(n)))


def check_momentum(m, before, after, impulse, iterations):
    """sum m v and sum (m x cross v - I w) before and after the pass, in float64.  The two ends of a pin are C apart, so its impulse
    pair carries the angular momentum C x P: that is taken off.  Every write of a velocity rounds it (two roundings per component),
    a body is written (iterations + 1) x its pins times: the bound is that many roundings of sum m |v| (sum m |x| |v| + I |w|)."""
    lin0, ang0 = ref.momenta(before)
    lin1, ang1 = ref.momenta(after)
    st = ref.State(before)
    pins = m.pins
    for k in range(len(pins)):
        c = ref._constraint(st, pins[k])[5]
        ang1 -= c[0] * float(impulse[k][1]) - c[1] * float(impulse[k][0])
    degree = np.bincount(np.concatenate([pins["body1"], pins["body2"]])).max()
    s_lin, s_ang = np.maximum(ref.momentum_scale(before), ref.momentum_scale(after))
    bound = 4 * U * (iterations + 1) * degree
    print("%s: linear %.3g of %.3g, angular %.3g of %.3g, bound %.3g" % (m.name, np.abs(lin1 - lin0).max(), s_lin, abs(ang1 - ang0), s_ang, bound))
    assert np.abs(lin1 - lin0).max() <= bound * s_lin
    assert abs(ang1 - ang0) <= bound * s_ang


INACTIVE = ("static_static", "static_world", "axle_world", "axle_centre", "axles_in_line")
