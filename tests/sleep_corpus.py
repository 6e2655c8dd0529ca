"""A directed corpus for the sleep pass (include/phyx_amd.h SLEEPING; the definition: tests/sleep_spec.py): the cases, what each one
reaches, and their premises.  test_sleep_corpus_cpu.py checks the premises without a GPU; test_sleep_corpus_gpu.py runs every case
on the device by twins (tests/sleep_lockstep.py), with no tolerance anywhere.

Part A, the graph cases, has no physics: gravity 0, boxes of half size 1 on a grid of pitch 40 (no two ever touch: no manifolds),
every velocity +0 unless the case sets one, and edges that exert nothing.  The default edge is a slack rope (a link with
min_length 0 and max_length 1e6): link_spec calls it idle and never solves it, whatever its bodies do, so a body that spins for ever
can hang on one.  A pin whose anchors coincide exerts nothing only as long as both bodies are at rest (a turning body swings the
anchor), so pins - and the inert angle and slider - stand in `every_kind` only, between bodies at rest.  The CPU file checks with
unit_spec that the pass leaves every body's bytes as they are.

A graph case is its edges, the velocities it starts with, the steps before which it zeroes some of them (`calms`), and k: the
tolerances are (0, 0, T) with T = ksum(k), float32(DT) added k times the way the spec's timer does.  What it expects comes from
components() and sleep_steps() below: a breadth-first search and one line of arithmetic that share nothing with sleep_spec.

Part B, the clauses that need a real step, are small scenes under gravity G; their runs are in the two test files.
"""
from collections import deque

import numpy as np

from phyx_amd import api
from unit_spec import KINDS
import sleep_spec

F = np.float32
DT = 1.0 / 60.0
G = -200.0
PITCH = 40.0
ROW = 64
SLEEP_WAVE_ROOTS = 4      # phyx_amd/csrc/sleep_kernels.h (test_sleep_corpus_cpu.py reads the header and compares)
CCW_BODIES = 256          # the compress windows of k_cc_compress_window, also the pass's workgroup size
WAVE = 64

# the clauses and paths the suite did not reach on the device: every one is named by at least one case's `reaches`
CLAUSES = ("struck sleepers", "sensor manifolds are no edge", "many roots in one wave", "labels on hard graphs",
           "the tie, the zeros and the denormals", "a unit that broke in this step is still an edge in it", "round bodies", "wake by list")


def ksum(k, dt=DT):
    """float32(dt) added k times from +0, as the spec's timer adds it"""
    t = F(0)
    for _ in range(k):
        t = F(t + F(dt))
    return t


def after(t):
    """the float32 above t"""
    return np.nextafter(F(t), F(np.inf))


def position(i):
    return PITCH * (i % ROW), PITCH * (i // ROW)


class GraphCase:
    """n bodies on the grid; `ropes`: (body1, body2) pairs; `others`: further units as lists(**others) of unit_lockstep takes them;
    `velocity`: {body: (vx, vy, w)} at the start; `calms`: {step: bodies whose velocity is zeroed before that step};
    `static`, `pinned`: as a scenes.py dict"""

    def __init__(self, name, n, ropes, reaches, k=3, velocity=None, calms=None, static=(), pinned=(), others=None):
        self.name, self.n, self.ropes, self.reaches, self.k = name, n, list(ropes), tuple(reaches), k
        self.velocity, self.calms = dict(velocity or {}), {int(s): list(b) for s, b in (calms or {}).items()}
        self.static, self.pinned, self.others = sorted(static), sorted(pinned), dict(others or {})

    # ---- what the worlds are built from ----
    def scene(self):
        i = np.arange(self.n)
        static, pinned = np.zeros(self.n, dtype=bool), np.zeros(self.n, dtype=bool)
        static[self.static] = True; pinned[self.pinned] = True
        return {"px": (PITCH * (i % ROW)).astype(np.float32), "py": (PITCH * (i // ROW)).astype(np.float32), "angle": np.zeros(self.n, dtype=np.float32),
                "sx": np.ones(self.n, dtype=np.float32), "sy": np.ones(self.n, dtype=np.float32), "static": static, "pinned": pinned}

    def lists(self):
        """one array per kind in the order of unit_spec.KINDS"""
        links = np.zeros(len(self.ropes), dtype=api.link_dtype)
        for j, (a, b) in enumerate(self.ropes):
            links[j]["body1"], links[j]["body2"], links[j]["max_length"] = a, b, 1e6
        given = dict(self.others)
        given["links"] = np.concatenate([links, given["links"]]) if "links" in given else links
        return [np.asarray(given.get(kind.plural, np.zeros(0, dtype=kind.dtype)), dtype=kind.dtype) for kind in KINDS]

    def pairs(self):
        return sleep_spec.unit_pairs(self.lists())

    def velocities(self):
        v = np.zeros((self.n, 3), dtype=np.float32)
        for b, x in self.velocity.items():
            v[b] = x
        return v

    def prepare(self, w):
        if self.velocity:
            named = sorted(self.velocity)
            w.set_velocities(named, self.velocities()[named])

    # ---- what it expects, by means of its own ----
    def mobile(self):
        m = np.ones(self.n, dtype=bool)
        m[self.static] = False
        return m

    def calm_from(self):
        """per body the first step in which its velocity is +0 or -0 or squares to 0 (None: never)"""
        out = []
        v = self.velocities()
        zeroed = {b: s for s in sorted(self.calms, reverse=True) for b in self.calms[s]}
        for b in range(self.n):
            calm = F(F(v[b, 0] * v[b, 0]) + F(v[b, 1] * v[b, 1])) <= 0 and F(v[b, 2] * v[b, 2]) <= 0
            out.append(0 if calm else zeroed.get(b))
        return out

    def sleep_steps(self):
        """{root: the step at whose end the component falls asleep (None: never)} - calm in k passes in a row, the last of its
        bodies to calm down deciding"""
        calm, out = self.calm_from(), {}
        for root, members in components(self.n, self.mobile(), self.pairs()).items():
            first = [calm[b] for b in members]
            out[root] = None if None in first else max(first) + self.k - 1
        return out

    def expected_slept(self, steps):
        """per step the ascending list of the bodies that fall asleep in it"""
        comp = components(self.n, self.mobile(), self.pairs())
        out = [[] for _ in range(steps)]
        for root, s in self.sleep_steps().items():
            if s is not None and s < steps:
                out[s] += comp[root]
        return [sorted(x) for x in out]


def components(n, mobile, pairs):
    """{smallest body: ascending members} of the graph on the mobile bodies: a breadth-first search"""
    near = [[] for _ in range(n)]
    for a, b in pairs:
        if 0 <= a < n and 0 <= b < n and mobile[a] and mobile[b]:
            near[a].append(b); near[b].append(a)
    seen, out = [False] * n, {}
    for start in range(n):
        if seen[start] or not mobile[start]:
            continue
        seen[start] = True
        members, queue = [], deque([start])
        while queue:
            x = queue.popleft()
            members.append(x)
            for y in near[x]:
                if not seen[y]:
                    seen[y] = True
                    queue.append(y)
        out[min(members)] = sorted(members)
    return out


def simulate(case, time_to_sleep, steps):
    """The spec alone on the case: nothing moves a body of a graph case, so a step leaves the velocities as they were.
    -> (per step the spec's slept list, the state after the last step)"""
    params = sleep_spec.Params(0.0, 0.0, time_to_sleep)
    state = sleep_spec.new_state(case.n)
    v = case.velocities()
    masses = np.ones((case.n, 2), dtype=np.float32)
    masses[case.static] = 0
    masses[case.pinned, 0] = 0
    units, none = case.pairs(), np.zeros(0, dtype=api.manifold_dtype)
    slept = []
    for s in range(steps):
        v[case.calms.get(s, [])] = 0
        got, woken = sleep_spec.decide(state, masses[:, 0], masses[:, 1], v[:, 0], v[:, 1], v[:, 2], none, units, None, params, DT)
        assert not woken
        masses[got] = 0; v[got] = 0
        slept.append(got)
    return slept, state


# ---- the graph cases ------------------------------------------------------------------------------------------------------------------
PATH_N, PATH_SEED, PATH_CUT, PATH_SPINNER = 1500, 20240, 600, 1000
SPIN = (0.0, 0.0, 1.0)


def path_order():
    return np.random.RandomState(PATH_SEED).permutation(PATH_N).tolist()


def permuted_path(k=3):
    """one component of 1500 bodies, a path through a random permutation: roots and windows in every order"""
    p = path_order()
    return GraphCase("permuted_path", PATH_N, zip(p[:-1], p[1:]), ("labels on hard graphs", "the tie, the zeros and the denormals", "wake by list"), k=k)


def cut_path():
    """the path without unit 600: parts of 601 and 899 bodies; one body of the larger part turns for ever"""
    p = path_order()
    ropes = [e for j, e in enumerate(zip(p[:-1], p[1:])) if j != PATH_CUT]
    return GraphCase("cut_path", PATH_N, ropes, ("labels on hard graphs",), velocity={p[PATH_SPINNER]: SPIN})


def star(high):
    """600 leaves; the hub is the largest index or index 0; the hub is body1 of every other rope"""
    hub, leaves = (600, range(600)) if high else (0, range(1, 601))
    return GraphCase("star_high" if high else "star_low", 601, [(hub, b) if b & 1 else (b, hub) for b in leaves], ("labels on hard graphs",))


# runs of consecutive indices (start, length): each length once from a multiple of 256 on and once from one past a multiple
RUNS = ((0, 255), (257, 255), (512, 256), (769, 256), (1280, 257), (1537, 257))
RUNS_N = 1794
RUN_AWAKE = 3            # the run that holds a body that never calms down, between runs that sleep
RUN_CUT = 2              # the run whose middle body test_sleep_corpus_gpu.py removes


def window_runs():
    """chains along runs of 255, 256 and 257 consecutive indices at and one past the window borders, each listed from its top down;
    the bodies between the runs are components of one"""
    ropes = []
    for start, length in RUNS:
        ropes += [(i, i - 1) for i in range(start + length - 1, start, -1)]
    start, length = RUNS[RUN_AWAKE]
    return GraphCase("window_runs", RUNS_N, ropes, ("labels on hard graphs", "wake by list"), velocity={start + length // 2: SPIN})


PAIRS_N = 1024
PAIRS_STATIC = 1024      # one static body behind the 1024, for the wake by list


def interleaved_pairs():
    """unit (i, i + 512): every aligned wave of 64 holds 64 components, each in two workgroups.  Component i calms down in step
    i % 4: never moving (0), body i turning until step 1, body i + 512 drifting until step 2, body i turning until step 3 - so in the
    upper waves the late timer is now the lane's own and now the partner's"""
    velocity, calms = {}, {1: [], 2: [], 3: []}
    for i in range(512):
        g = i % 4
        if g:
            b = i + 512 if g == 2 else i
            velocity[b] = (0.5, 0.0, 0.0) if g == 2 else SPIN
            calms[g].append(b)
    return GraphCase("interleaved_pairs", PAIRS_N + 1, [(i, i + 512) for i in range(512)], ("many roots in one wave", "wake by list"),
                     velocity=velocity, calms=calms, static=[PAIRS_STATIC])


def wave_premise(slept):
    """-> (the aligned block of 64 indices, its components, their sleep steps) with the most components that fell asleep, over the
    blocks whose components fell asleep in at least three different steps; `slept`: per step the bodies that fell asleep"""
    step_of = {b: s for s, bodies in enumerate(slept) for b in bodies}
    best = (None, [], set())
    for block in range(0, PAIRS_N, WAVE):
        roots = sorted({b % 512 for b in range(block, block + WAVE) if b in step_of})
        steps = {step_of[r] for r in roots}
        if len(steps) >= 3 and len(roots) > len(best[1]):
            best = (block, roots, steps)
    return best


def every_kind():
    """a chain 0 .. 4 of one unit of each kind - a pin whose anchors coincide, a slack rope, an angle without a row (limits wider than
    a turn), a slider at rest on its rail inside its limits - and two bodies tied to the world only: 5 by a pin through its centre,
    turning for ever, 6 by a slack rope, at rest"""
    x = lambda i: position(i)[0]
    pins = np.zeros(2, dtype=api.pin_dtype)
    pins[0] = (0, 1, (0.0, 0.0), (x(0) - x(1), 0.0), (0.0, 0.0))
    pins[1] = (5, -1, (0.0, 0.0), position(5), (0.0, 0.0))
    links = np.zeros(1, dtype=api.link_dtype)
    links[0]["body1"], links[0]["body2"], links[0]["anchor2"], links[0]["max_length"] = 6, -1, position(6), 1e6
    angles = np.zeros(1, dtype=api.angle_dtype)
    angles[0]["body1"], angles[0]["body2"], angles[0]["lower"], angles[0]["upper"] = 2, 3, -10.0, 10.0
    sliders = np.zeros(1, dtype=api.slider_dtype)
    sliders[0]["body1"], sliders[0]["body2"], sliders[0]["anchor2"], sliders[0]["axis"] = 3, 4, (x(3) - x(4), 0.0), (1.0, 0.0)
    sliders[0]["lower"], sliders[0]["upper"] = -1e3, 1e3
    return GraphCase("every_kind", 7, [(1, 2)], ("labels on hard graphs",), velocity={5: SPIN},
                     others=dict(pins=pins, links=links, angles=angles, sliders=sliders))


# zeros: body -> its velocity; 1e-20 squares to a float32 denormal (above 0: not calm), 1e-23 squares to +0 (calm)
NEG0 = F(-0.0)
ZEROS = {0: (NEG0, NEG0, NEG0), 1: (1e-20, 0.0, 0.0), 2: (1e-23, 0.0, 0.0), 3: (0.0, 0.0, 1e-20), 4: (0.0, 0.0, 1e-23), 5: (0.0, 1e-20, 0.0), 6: (0.0, 0.0, 0.0)}
ZEROS_CALM, ZEROS_NOT = [0, 2, 4, 6], [1, 3, 5]


ZEROS_KEEP = F(-1e-45)      # the smallest negative denormal


def zeros():
    """seven bodies on their own.  Body 0 carries -0.0 in all three words.  IntegrateVelocity computes v + a dt, and with a = +0 that
    turns -0 into +0: no -0.0 survives a plain step, and add_accelerations cannot hand over a = -0 either (it adds to the +0 that is
    there).  So body 0 has inverse mass 0 (gravity is not added to its acceleration) and the test gives it the acceleration ZEROS_KEEP
    in all three words before every step: a dt underflows to -0, and (-0) + (-0) stays -0.  The test asserts on world B that it did."""
    return GraphCase("zeros", 7, [], ("the tie, the zeros and the denormals",), velocity=ZEROS, pinned=[0])


def graph_cases():
    return [permuted_path(), cut_path(), star(True), star(False), window_runs(), interleaved_pairs(), every_kind(), zeros()]


# ---- Part B: scenes under gravity ---------------------------------------------------------------------------------------------------------
GENEROUS = (20.0, 5.0)      # tolerances far above what a resting box has (test_sleep_gpu.py): calm from the first step


def rows_scene(rows, pinned=()):
    """rows (px, py, half_x, half_y, static) -> a scenes.py dict"""
    r = np.asarray([row[:4] for row in rows], dtype=np.float32).reshape(-1, 4)
    p = np.zeros(len(rows), dtype=bool)
    p[list(pinned)] = True
    return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": np.zeros(len(rows), dtype=np.float32), "sx": r[:, 2].copy(), "sy": r[:, 3].copy(),
            "static": np.asarray([bool(row[4]) for row in rows], dtype=bool), "pinned": p}


# struck: the ground with a column of three and two more platforms with a column each, 100 apart
PLATFORMS = (0, 4, 8)


def column(c):
    return [PLATFORMS[c] + 1 + r for r in range(3)]


def platforms():
    rows = []
    for cx in (0.0, 100.0, -100.0):
        rows.append((cx, 0.0, 15.0, 10.0, True))
        rows += [(cx, 15.0 + 10.0 * r, 5.0, 5.0, False) for r in range(3)]
    return rows_scene(rows)


# (the step before which it is given, the platform, its velocity, whether it strikes).  The -0.0 does not: a platform that shares a manifold
# with points with anybody has a contact joint, and the step's solver leaves +0 where the -0.0 was (v + 0 * impulse), so the word the pass
# sees is 0 - on the oracle and, asserted there on world B, on the device.  "A -0.0 strikes" is reachable on fabricated states only
# (test_sleep_cpu.py); what a real step can hold is a denormal: 1e-40 moves nothing and strikes
STRUCK = {"reaches": ("struck sleepers",), "params": GENEROUS + (ksum(3),), "sleep_step": 2,
          "strikes": ((4, 4, (3.0, 0.0, 0.0), True), (5, 8, (NEG0, 0.0, 0.0), False), (6, 0, (0.0, 0.0, 1e-3), True), (7, 8, (0.0, 1e-40, 0.0), True))}

# sensor: a column of three on the ground and a box that turns in place (inverse mass 0) across the top box, a sensor until step 5
SENSOR_BODY, SENSOR_SPIN, SENSOR_COLUMN = 4, (0.0, 0.0, 6.0), [1, 2, 3]
SENSOR = {"reaches": ("sensor manifolds are no edge",), "params": GENEROUS + (ksum(3),), "sleep_step": 2, "clear_before": 5}


def sensor_scene():
    return rows_scene([(0.0, 0.0, 15.0, 10.0, True)] + [(0.0, 15.0 + 10.0 * r, 5.0, 5.0, False) for r in range(3)] + [(3.0, 38.0, 4.0, 4.0, False)], pinned=[SENSOR_BODY])


# broken_this_step: box 1 rests on the ground; box 2 hangs beside it, above the ground, from a pin through its own centre, and turns
# faster than the angular tolerance for ever (the pin's anchor is its centre: nothing slows it).  The pin is unbreakable for two steps
# and gets a limit far below the weight it carries before step 2: it breaks in that step's pass, in which box 1's timer reaches T
BROKEN = {"reaches": ("a unit that broke in this step is still an edge in it",), "params": GENEROUS + (ksum(3),), "break_step": 2, "limit": 1e-3,
          "a": 1, "b": 2, "spin": (0.0, 0.0, 6.0)}


def broken_scene():
    return rows_scene([(0.0, 0.0, 30.0, 10.0, True), (0.0, 15.0, 5.0, 5.0, False), (12.0, 15.0, 2.0, 2.0, False)])


def broken_pins():
    p = np.zeros(1, dtype=api.pin_dtype)
    p[0] = (1, 2, (12.0, 0.0), (0.0, 0.0), (0.0, 0.0))
    return p


# round: two boxes 4 apart on the ground, a circle of radius 4 in the notch between them, a circle of radius 3 rolling on the ground
ROUND = {"reaches": ("round bodies",), "params": (6.0, 3.0, ksum(3)), "pile": [1, 2, 3], "roller": 4, "circles": ([3, 4], [4.0, 3.0]),
         "roll": (10.0, 0.0, -10.0 / 3.0), "drop": (0.0, 32.0, 0.0, 3.0), "drop_velocity": (0.0, -30.0, 0.0)}


def round_scene():
    return rows_scene([(0.0, 0.0, 80.0, 10.0, True), (-7.0, 15.0, 5.0, 5.0, False), (7.0, 15.0, 5.0, 5.0, False), (0.0, 23.5, 4.0, 4.0, False),
                       (30.0, 13.0, 3.0, 3.0, False)])


# ---- the table: which case reaches which clause -------------------------------------------------------------------------------------------
def table():
    """{case: the clauses of CLAUSES it reaches}"""
    t = {c.name: c.reaches for c in graph_cases()}
    t.update(tie=("the tie, the zeros and the denormals",), wake_by_list=("wake by list",), struck=STRUCK["reaches"], sensor=SENSOR["reaches"],
             broken_this_step=BROKEN["reaches"], round=ROUND["reaches"])
    return t
