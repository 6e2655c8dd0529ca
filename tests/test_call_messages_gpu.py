"""The text of the refusals of the between-step calls for pins, links and the per-body columns (include/phyx_amd.h PINS, LINKS,
COLLISION FILTERS, MATERIALS, BODY FLAGS): status and phx_last_error, word for word, and the world unchanged after each.  The status
codes are covered where each call is tested; the messages carry the call's name and the record's noun, which is what a shared
implementation of the calls could mix up.  The order of the checks shows where two refusals apply at once: a column setter on a
sharded world inside a step gives the sharded message, a unit call there the mid-step one."""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, PhxError, scenes
from phyx_amd.api import angle_dtype, link_dtype, pin_dtype, slider_dtype

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
INVALID, CAPACITY, STATE = -1, -4, -5
NAN = float("nan")
MID_STEP = ": the world is between pre_solve / step_begin and finish_step / step_end"
DTYPES = {"pin": pin_dtype, "link": link_dtype}
GOOD = {"pin": (0, 1, (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)), "link": (0, 1, (1.0, 0.0), (0.0, 1.0), 2.0, 3.0, 0.0, 0.0, 0.0, 0)}
# scenes.stack(2, 3): the ground and two columns of three boxes, 7 bodies
PINS = np.array([(1, 2, (0.0, 5.0), (0.0, -5.0), (0.0, 0.0)), (6, -1, (0.0, 0.0), (0.0, 35.0), (0.0, 0.0))], dtype=pin_dtype)
LINKS = np.array([(2, 3, (0.0, 0.0), (0.0, 0.0), 10.0, 10.0, 0.0, 0.0, 0.0, 0),                  # link 0: a rod
                  (4, -1, (0.0, 0.0), (0.0, 35.0), 20.0, 20.0, 2.0, 0.5, 0.0, 0)], dtype=link_dtype)      # link 1: a spring


def _cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, 15, 15)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _world(pins=PINS, links=LINKS):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 3))
    pw.add_pins(pins)
    pw.add_links(links)
    return pw


def _recs(kind, **fields):
    """two good records of `kind`, the second with `fields` changed (a tuple: (component, value))"""
    p = np.array([GOOD[kind], GOOD[kind]], dtype=DTYPES[kind])
    for f, v in fields.items():
        if isinstance(v, tuple):
            p[f][1][v[0]] = v[1]
        else:
            p[f][1] = v
    return p


def _add(pw, kind, recs, count=None, null=False):
    return getattr(pw.L, "phx_world_add_%ss" % kind)(pw.h, None if null else vp(recs), len(recs) if count is None else count, None)


def _get(pw, kind, cap):
    out = np.zeros(8, dtype=DTYPES[kind])
    return getattr(pw.L, "phx_world_get_%ss" % kind)(pw.h, vp(out), cap)


def _anchors(*rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 4)


def _lengths(*rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 2)


def _refusal(pw, call):
    """-> (status, message) of a call that goes through the Python API (PhxError) or straight to the C ABI (a status)"""
    try:
        st = call(pw)
    except PhxError as e:
        prefix = "libphyx_amd: status %d: " % e.status
        assert str(e).startswith(prefix)
        return e.status, str(e)[len(prefix):]
    return st, pw.L.phx_last_error().decode()


def _snapshot(pw):
    return pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.pin_schedule_builds()


def _refused(pw, cases):
    before = _snapshot(pw)
    for name, call, status, message in cases:
        got = _refusal(pw, call)
        print(name, "->", got)
        assert got == (status, message), name
        assert _snapshot(pw) == before, "the world changed: " + name


# (name, call, status, message) per kind; entry 1 of an add is the bad one
UNIT_CASES = {
    "pin": [
        ("add, negative count", lambda w: _add(w, "pin", _recs("pin"), count=-1), INVALID, "phx_world_add_pins: negative count -1"),
        ("add, null array", lambda w: _add(w, "pin", _recs("pin"), null=True), INVALID, "phx_world_add_pins: null array"),
        ("add, body1 = -1", lambda w: _add(w, "pin", _recs("pin", body1=-1)), INVALID, "phx_world_add_pins: pin 1: body1 -1 out of range [0, 7)"),
        ("add, body2 = -2", lambda w: _add(w, "pin", _recs("pin", body2=-2)), INVALID, "phx_world_add_pins: pin 1: body2 -2 is neither -1 nor in [0, 7)"),
        ("add, body1 == body2", lambda w: _add(w, "pin", _recs("pin", body1=2, body2=2)), INVALID, "phx_world_add_pins: pin 1: both ends on body 2"),
        ("add, NaN anchor", lambda w: _add(w, "pin", _recs("pin", anchor1=(1, NAN))), INVALID, "phx_world_add_pins: pin 1: value 1 is not finite"),
        ("remove, out of range", lambda w: w.remove_pins([2]), INVALID, "phx_world_remove_pins: pin index 2 out of range [0, 2)"),
        ("remove, duplicate", lambda w: w.remove_pins([1, 1]), INVALID, "phx_world_remove_pins: pin 1 appears twice in one call"),
        ("set anchors, NaN", lambda w: w.set_pin_anchors([0], _anchors([0.0, NAN, 0.0, 0.0])), INVALID, "phx_world_set_pin_anchors: entry 0: value 1 is not finite"),
        ("get, cap = 0", lambda w: _get(w, "pin", 0), CAPACITY, "phx_world_get_pins: room for 0 pins, the world has 2"),
    ],
    "link": [
        ("add, negative count", lambda w: _add(w, "link", _recs("link"), count=-1), INVALID, "phx_world_add_links: negative count -1"),
        ("add, null array", lambda w: _add(w, "link", _recs("link"), null=True), INVALID, "phx_world_add_links: null array"),
        ("add, body1 = -1", lambda w: _add(w, "link", _recs("link", body1=-1)), INVALID, "phx_world_add_links: link 1: body1 -1 out of range [0, 7)"),
        ("add, body2 = -2", lambda w: _add(w, "link", _recs("link", body2=-2)), INVALID, "phx_world_add_links: link 1: body2 -2 is neither -1 nor in [0, 7)"),
        ("add, body1 == body2", lambda w: _add(w, "link", _recs("link", body1=2, body2=2)), INVALID, "phx_world_add_links: link 1: both ends on body 2"),
        ("add, NaN anchor", lambda w: _add(w, "link", _recs("link", anchor1=(1, NAN))), INVALID, "phx_world_add_links: link 1: value 1 is not finite"),
        ("remove, out of range", lambda w: w.remove_links([2]), INVALID, "phx_world_remove_links: link index 2 out of range [0, 2)"),
        ("remove, duplicate", lambda w: w.remove_links([1, 1]), INVALID, "phx_world_remove_links: link 1 appears twice in one call"),
        ("set anchors, NaN", lambda w: w.set_link_anchors([0], _anchors([0.0, NAN, 0.0, 0.0])), INVALID, "phx_world_set_link_anchors: entry 0: value 1 is not finite"),
        ("get, cap = 0", lambda w: _get(w, "link", 0), CAPACITY, "phx_world_get_links: room for 0 links, the world has 2"),
        ("set lengths, min > max", lambda w: w.set_link_lengths([0], _lengths([3.0, 2.0])), INVALID,
         "phx_world_set_link_lengths: link 0: lengths [3, 2] are not 0 <= min <= max"),
        ("set lengths, a spring with min != max", lambda w: w.set_link_lengths([1], _lengths([1.0, 2.0])), INVALID,
         "phx_world_set_link_lengths: link 0: a spring (hertz 2) needs min_length == max_length"),
        ("add, reserved = 1", lambda w: _add(w, "link", _recs("link", reserved=1)), INVALID, "phx_world_add_links: link 1: reserved must be 0"),
        ("add, negative hertz", lambda w: _add(w, "link", _recs("link", hertz=-1.0)), INVALID, "phx_world_add_links: link 1: negative hertz or damping_ratio"),
    ],
}
# the calls a step refuses (the getters are not among them)
UNIT_CALLS = {
    "pin": [
        ("phx_world_add_pins", lambda w: w.add_pins(_recs("pin"))),
        ("phx_world_remove_pins", lambda w: w.remove_pins([0])),
        ("phx_world_set_pin_anchors", lambda w: w.set_pin_anchors([0], _anchors([0.0, 0.0, 0.0, 0.0]))),
    ],
    "link": [
        ("phx_world_add_links", lambda w: w.add_links(_recs("link"))),
        ("phx_world_remove_links", lambda w: w.remove_links([0])),
        ("phx_world_set_link_anchors", lambda w: w.set_link_anchors([0], _anchors([0.0, 0.0, 0.0, 0.0]))),
        ("phx_world_set_link_lengths", lambda w: w.set_link_lengths([0], _lengths([5.0, 5.0]))),
    ],
}
SHARDED = {
    "pin": ("phx_world_add_pins: a sharded world carries no pins", "phx_world_set_shard: the world holds pins, which a sharded world does not carry"),
    "link": ("phx_world_add_links: a sharded world carries no links", "phx_world_set_shard: the world holds links, which a sharded world does not carry"),
}


@pytest.mark.parametrize("staged", ["host", "device"])
@pytest.mark.parametrize("kind", ["pin", "link"])
def test_unit_calls_refuse_in_these_words(built_lib, kind, staged):
    cfg = _cfg()
    pw = _world()
    if staged == "device":
        pw.Update(DT, cfg)
    _refused(pw, UNIT_CASES[kind])
    pw.PreSolve(DT)
    _refused(pw, [("in a step: " + what, call, STATE, what + MID_STEP) for what, call in UNIT_CALLS[kind]])
    pw.FinishStep(DT, cfg)
    assert (pw.pin_count(), pw.link_count()) == (2, 2)


@pytest.mark.parametrize("kind", ["pin", "link"])
def test_sharded_worlds_refuse_units_in_these_words(built_lib, kind):
    add_message, shard_message = SHARDED[kind]
    sharded = _world(PINS[:0], LINKS[:0])
    sharded.set_shard(0, 2)
    _refused(sharded, [("add on a sharded world", UNIT_CALLS[kind][0][1], STATE, add_message)])
    # (a world with both names its pins)
    holder = _world(PINS if kind == "pin" else PINS[:0], LINKS)
    _refused(holder, [("set_shard on a world with units", lambda w: w.set_shard(0, 2), STATE, shard_message)])
    if kind == "pin":
        _refused(_world(PINS, LINKS[:0]), [("set_shard on a world with pins alone", lambda w: w.set_shard(0, 2), STATE, shard_message)])


# (the call's name, its refusal on a sharded world, the call on body 1)
COLUMN_CALLS = [
    ("phx_world_set_collision_filters", "phx_world_set_collision_filters: a sharded world carries no collision filters", lambda w: w.set_collision_filters([1], category=2)),
    ("phx_world_set_materials", "phx_world_set_materials: a sharded world carries no materials", lambda w: w.set_materials([1], friction=0.5)),
    ("phx_world_set_body_flags", "phx_world_set_body_flags: a sharded world carries no body flags", lambda w: w.set_body_flags([1], 1)),
]
COLUMN_CASES = [
    ("filters, a body twice", lambda w: w.set_collision_filters([1, 2, 1], category=2), INVALID, "phx_world_set_collision_filters: body 1 appears twice in one call"),
    ("materials, a body twice", lambda w: w.set_materials([1, 2, 1], friction=0.5), INVALID, "phx_world_set_materials: body 1 appears twice in one call"),
    ("flags, a body twice", lambda w: w.set_body_flags([1, 2, 1], 1), INVALID, "phx_world_set_body_flags: body 1 appears twice in one call"),
    ("friction = -1", lambda w: w.set_materials([2, 1], friction=[0.5, -1.0]), INVALID, "phx_world_set_materials: friction -1 of body 1 is not in [0, 1e6]"),
    ("restitution = 2", lambda w: w.set_materials([2, 1], restitution=[0.5, 2.0]), INVALID, "phx_world_set_materials: restitution 2 of body 1 is not in [0, 1]"),
    ("an unknown flag bit", lambda w: w.set_body_flags([2, 1], [1, 2]), INVALID, "phx_world_set_body_flags: flags 0x2 of body 1 hold an unknown bit"),
]


def _columns(pw):
    return pw.collision_filters().tobytes(), pw.materials().tobytes(), pw.body_flags().tobytes()


@pytest.mark.parametrize("staged", ["host", "device"])
def test_column_setters_refuse_in_these_words(built_lib, staged):
    cfg = _cfg()
    pw = _world()
    pw.set_materials([3], friction=0.25)                                    # (an active table and two that are not)
    if staged == "device":
        pw.Update(DT, cfg)
    columns = _columns(pw)
    _refused(pw, COLUMN_CASES)
    assert _columns(pw) == columns
    pw.PreSolve(DT)
    _refused(pw, [("in a step: " + what, call, STATE, what + MID_STEP) for what, _, call in COLUMN_CALLS])
    pw.FinishStep(DT, cfg)
    assert _columns(pw) == columns


def test_sharded_worlds_refuse_columns_in_these_words(built_lib):
    """... before anything else: also inside a step (step_begin), where a unit call names the step"""
    from phyx_amd.dist import Exchange
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE)
    cases = [(what, call, STATE, sharded) for what, sharded, call in COLUMN_CALLS]
    units = [("in a step: " + what, call, STATE, what + MID_STEP) for kind in ("pin", "link") for what, call in UNIT_CALLS[kind][:1]]
    cap = Exchange.capacity_for(7, 56)
    worlds, send, recv = [], [], []
    for r in range(2):
        w = _world(PINS[:0], LINKS[:0])
        w.set_shard(r, 2)
        send.append(phyx_amd.DeviceBuffer(cap, 0)); recv.append(phyx_amd.DeviceBuffer(2 * cap, 0))
        w.solver.set_exchange_buffers(send[r].ptr.value, recv[r].ptr.value, cap)
        worlds.append(w)
    _refused(worlds[0], cases)
    segs = [w.StepBegin(DT, cfg) for w in worlds]
    assert segs[0] == segs[1]
    for name, call, status, message in cases + units:
        assert _refusal(worlds[0], call) == (status, message), "in a sharded step: " + name
    for w in worlds:
        w.sync()
    for dst in range(2):
        for src in range(2):
            recv[dst].copy_from(send[src], segs[0], dst_offset=src * segs[0], stream=worlds[dst].stream_ptr())
    for w in worlds:
        w.StepEnd(DT)
    assert _snapshot(worlds[0]) == _snapshot(worlds[1]), "the refused calls left the rank as its twin"


# ---- the limit and motor rules of angles and sliders: one rule for an add and for the set call, one text per kind ----
LIMITED = {"angle": dict(dtype=angle_dtype, bound="max_torque", first_float=0,      # (`first_float`: value 0 of the add's finite check is `lower` behind this many floats)
                         good=(0, 1, -0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), spring=(0, 1, 0.1, 0.1, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0)),
           "slider": dict(dtype=slider_dtype, bound="max_force", first_float=6,
                          good=(0, 1, (0.0, 0.0), (0.0, 0.0), (1.0, 0.0), -0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0),
                          spring=(0, 1, (0.0, 0.0), (0.0, 0.0), (1.0, 0.0), 0.1, 0.1, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0))}


@pytest.mark.parametrize("kind", ["angle", "slider"])
def test_limit_and_motor_rules_refuse_in_these_words(built_lib, kind):
    """Every text of the limits' rule (not finite, not lower <= upper, a spring needs lower == upper) and of the motor's (not finite,
    a negative bound), whole, through the add and through the set call, on one world of two bodies with one call per case.  An add
    checks that every float is finite before it looks at a rule, so there the two `not finite` texts are the finite check's own."""
    K = LIMITED[kind]
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(1, 1))
    assert pw.counts()[0] == 2
    getattr(pw, "add_%ss" % kind)(np.array([K["good"], K["spring"]], dtype=K["dtype"]))      # unit 0: limits, unit 1: a spring
    records = lambda: getattr(pw, "%ss" % kind)().tobytes()
    before = records()

    def add(**fields):
        p = np.array([K["good"], K["good"]], dtype=K["dtype"])
        for f, v in fields.items():
            p[f][1] = v
        return getattr(pw.L, "phx_world_add_%ss" % kind)(pw.h, vp(p), 2, None)

    def set_(what, which, values):
        idx, v = np.array([which], dtype=np.int32), np.array([values], dtype=np.float32)
        return getattr(pw.L, "phx_world_set_%s_%s" % (kind, what))(pw.h, vp(idx), vp(v), 1)

    A = "phx_world_add_%ss: %s 1: " % (kind, kind)
    L = "phx_world_set_%s_limits: %s 0: " % (kind, kind)
    M = "phx_world_set_%s_motors: %s 0: " % (kind, kind)
    bound, f0 = K["bound"], K["first_float"]
    cases = [(lambda: add(lower=NAN), A + "value %d is not finite" % f0), (lambda: add(upper=np.inf), A + "value %d is not finite" % (f0 + 1)),
             (lambda: add(lower=1.0), A + "limits [1, 0.5] are not lower <= upper"),
             (lambda: add(hertz=2.0), A + "a spring (hertz 2) needs lower == upper"),
             (lambda: add(motor_speed=np.inf), A + "value %d is not finite" % (f0 + 4)), (lambda: add(**{bound: NAN}), A + "value %d is not finite" % (f0 + 5)),
             (lambda: add(**{bound: -1.0}), A + "negative %s -1" % bound),
             (lambda: set_("limits", 0, [NAN, 1.0]), L + "a limit is not finite"), (lambda: set_("limits", 0, [1.0, np.inf]), L + "a limit is not finite"),
             (lambda: set_("limits", 0, [3.0, 2.0]), L + "limits [3, 2] are not lower <= upper"),
             (lambda: set_("limits", 1, [1.0, 2.0]), L + "a spring (hertz 2) needs lower == upper"),
             (lambda: set_("motors", 0, [np.inf, 1.0]), M + "a motor value is not finite"), (lambda: set_("motors", 0, [1.0, NAN]), M + "a motor value is not finite"),
             (lambda: set_("motors", 0, [1.0, -2.0]), M + "negative %s -2" % bound)]
    for call, message in cases:
        got = (call(), pw.L.phx_last_error().decode())
        print(got)
        assert got == (INVALID, message)
        assert records() == before, "the world changed: " + message
    assert set_("limits", 1, [0.25, 0.25]) == 0 and set_("motors", 0, [1.0, 0.0]) == 0, "a spring with lower == upper and a motor bound of 0 are fine"

