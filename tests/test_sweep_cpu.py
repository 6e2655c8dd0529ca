"""Continuous bodies without a GPU (include/phyx_amd.h CONTINUOUS BODIES):
  - tests/sweep_spec.py, the float32 definition, against tests/sweep_reference.py, its float64 judge, on tests/sweep_corpus.py;
  - the corpus reaches every arm of the rule;
  - phx_continuous_check, the host check behind every refusal of phx_world_set_continuous that concerns the radius, message by message."""
import numpy as np
import pytest

import phyx_amd
import polygon_spec as ps
import round_query_corpus as rqc
import sweep_corpus as sc
import sweep_reference as ref
import sweep_spec as spec
from phyx_amd import PhxError, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_CIRCLE, SHAPE_POLYGON

F = np.float32
# The bounds, in u = 2^-24 * scale, are the circle casts' own (tests/round_query_corpus.py): 16 u for every measure; for a target with
# faces (a box, and a polygon, whose pushed-out faces and vertex arcs are met exactly as a box's are) the entry's 64 u and the
# normal's 128 u, the grazing-angle term explained there.  The polygon rule stays inside them: the worst the specification measures
# against the judge on this corpus is printed by the test below (hit 2.5 u, normal 3.7 u, length 1.6 u when this was written).
FACED = (sc.BOX, sc.POLYGON)


def _bound(kind, measure):
    return rqc.BOUNDS.get(("box", measure), rqc.BOUND) if kind in FACED else rqc.BOUND


def _run(c, detail=None):
    return spec.sweep(c.bodies, c.start, c.rc, c.kinds, c.polys, c.flags, c.filters, c.exclusions, detail=detail)


def _expected(c, hits, labels):
    target, label = c.want
    if target is None:
        if len(hits):
            return False
        return label is None or any(l == label or (isinstance(l, tuple) and l[0] == label) for l in labels.values())
    return len(hits) == 1 and int(hits[0]["target"]) == target and int(hits[0]["body"]) == c.mover and (label is None or labels[target] == label)


def test_the_ill_conditioned_cases_are_named_and_few():
    names = {c.name for c in sc.cases()}
    assert set(sc.ILL) <= names
    assert len(sc.ILL) <= 0.05 * len(names), "%d of %d cases are left out of the judgement" % (len(sc.ILL), len(names))


def test_spec_against_the_float64_judge():
    """Every case but the named ill-conditioned ones: every (swept body, target) pair the rule considers gets the judge's verdict
    (overlap, miss or hit), and the winner's t and normal are the judge's within the circle casts' bounds.  The judge must itself call a
    case it is asked about well conditioned: a clearance above NEAR u."""
    worst = {}
    for c in sc.cases():
        if c.name in sc.ILL or c.name in sc.RULE_ONLY:
            continue
        detail = {}
        out, hits = _run(c, detail)
        i = c.mover
        s, rc = c.start[i], c.rc[i]
        d = (F(c.bodies[i]["pos"]["x"]) - s[0], F(c.bodies[i]["pos"]["y"]) - s[1])
        if d[0] == 0 and d[1] == 0:
            assert not len(hits)
            continue
        considered = spec.targets(c.bodies, i, c.flags, c.filters, c.exclusions)
        verdicts = {}
        for j in np.flatnonzero(considered):
            t = ref.Target(c.bodies[j], c.kinds[j], c.polys[j])
            v = ref.cast(t, s, rc, d)
            verdicts[int(j)] = (t, v)
            assert v.clearance > ref.NEAR * ref.unit(t, s, rc, d, v.t or 0.0), "%s: the judge calls target %d ill conditioned (clearance %.3g)" % (c.name, j, v.clearance)
            label = detail[i].get(int(j))                                   # (None: no hit, the AABB conjunct included)
            got = "overlap" if label == "overlap" else ("miss" if label is None else "hit")
            assert got == v.kind, "%s: target %d is a %s to the rule (%s) and a %s to the judge" % (c.name, j, got, label, v.kind)
        judged = [(v.t, j) for j, (t, v) in verdicts.items() if v.kind == "hit"]
        if not judged:
            assert not len(hits), c.name
            continue
        assert len(hits) == 1, c.name
        tmin = min(t for t, _ in judged)
        assert int(hits[0]["target"]) in [j for t, j in judged if t == tmin], "%s: the rule hits %d, the judge %s" % (c.name, hits[0]["target"], judged)
        j = int(hits[0]["target"])
        t, v = verdicts[j]
        u = ref.unit(t, s, rc, d, v.t)
        touch = detail[("touch", i)]                                        # (the first touch: the judge's t; the hit records t', a skin short of it)
        for m, figure in ref.deviation(t, rc, d, v, touch, hits[0]["normal"]).items():
            key = ("faced" if c.kinds[j] in FACED else "round", m)
            if figure / u > worst.get(key, (0.0, ""))[0]:
                worst[key] = (figure / u, c.name)
            assert figure / u <= _bound(c.kinds[j], m), "%s: %s is %.3g u, the bound is %g u" % (c.name, m, figure / u, _bound(c.kinds[j], m))
        # the skin: t' = max(touch - skin / approach, 0), and the position the pass leaves: s + d*t', one rounding per operation
        n = hits[0]["normal"]
        back = F(touch - F(spec.skin(rc) / -(F(n[0] * d[0]) + F(n[1] * d[1]))))
        assert hits[0]["t"] == (back if back > 0 else F(0)) and hits[0]["t"] <= touch
        assert out[i]["pos"]["x"] == F(s[0] + F(d[0] * hits[0]["t"])) and out[i]["pos"]["y"] == F(s[1] + F(d[1] * hits[0]["t"]))
    print("worst in u: " + "  ".join("%s %s %.3g (%s)" % (k[0], k[1], v[0], v[1]) for k, v in sorted(worst.items())))


def test_the_corpus_reaches_every_arm():
    labels, winners = {k: set() for k in range(4)}, {k: set() for k in range(4)}
    for c in sc.cases():
        detail = {}
        out, hits = _run(c, detail)
        assert _expected(c, hits, detail.get(c.mover, {})), "%s: wanted %s, got %s with %s" % (c.name, c.want, hits, detail)
        for j, l in detail.get(c.mover, {}).items():
            labels[int(c.kinds[j])].add(l)
        for h in hits:
            winners[int(c.kinds[h["target"]])].add(detail[c.mover][int(h["target"])])
        # a body the pass does not clamp keeps its bytes
        if not len(hits):
            assert out.tobytes() == c.bodies.tobytes(), c.name
    assert winners[sc.BOX] >= {(0, "x"), (1, "y"), 2, 3, 4, 5}, winners[sc.BOX]
    assert winners[sc.CIRCLE] >= {6}
    assert winners[sc.CAPSULE] >= {"side+", "side-", "end0", "end1"}, winners[sc.CAPSULE]
    tri = {c.want[1] for c in sc.cases() if c.name.startswith(("triangle-face", "triangle-vertex"))}
    octa = {c.want[1] for c in sc.cases() if c.name.startswith(("octagon-face", "octagon-vertex"))}
    assert tri == {("face", k) for k in range(3)} | {("vertex", k) for k in range(3)}
    assert octa == {("face", k) for k in range(8)} | {("vertex", k) for k in range(8)}
    assert winners[sc.POLYGON] >= octa
    for kind in range(4):
        assert "overlap" in labels[kind], "no start overlap against kind %d" % kind
    assert any(isinstance(l, tuple) and l[0] == "away" for l in labels[sc.BOX])
    for name in ("t-exactly-0", "held-a-skin-short"):
        h = _run(sc.case(name))[1]
        assert len(h) == 1 and h[0]["t"].tobytes() == F(0).tobytes(), name
    detail = {}
    h = _run(sc.case("t-exactly-1"), detail)[1]
    assert len(h) == 1 and detail[("touch", 1)] == F(1) and h[0]["t"] == F(1 - 0.0078125)      # the touch at t = 1, the body a skin (of rc 0.5, |d| 1) short
    assert not len(_run(sc.case("d-is-zero"))[1])


def test_the_skin_arms():
    """The two places the skin enters the rule, against stated expectations (the judge knows no skin).  rc = 0.5: the skin is 2^-7."""
    skin = F(0.0078125)
    assert spec.skin(0.5) == skin
    # a step that approaches by less than the skin is no hit, though the core would enter: 0.006 < skin < 0.009
    detail = {}
    assert not len(_run(sc.case("creeping-in"), detail)[1]) and detail[1][0] == ("away", (0, "x"))
    h = _run(sc.case("just-faster-than-creeping"))[1]
    assert len(h) == 1 and h[0]["target"] == 0
    # a clamped body stands a skin short of the touch, measured along the normal: the box's face is at -1, the core's radius 0.5
    for name in ("t-exactly-1", "box-(0, 'x')@0"):
        c = sc.case(name)
        out, h = _run(c)
        gap = -1.0 - float(c.rc[c.mover]) - float(out[c.mover]["pos"]["x"]) if name != "box-(0, 'x')@0" else -2.0 - 0.4 - float(out[c.mover]["pos"]["x"])
        assert abs(gap - float(spec.skin(c.rc[c.mover]))) < 1e-6, (name, gap)
    # ... and from there a fast step is held at t' = 0, a creeping one is let go, one that leaves is not looked at
    c = sc.case("held-a-skin-short")
    out, h = _run(c)
    assert len(h) == 1 and h[0]["t"] == 0 and out[1]["pos"]["x"] == c.start[1][0]


def test_a_swept_body_that_is_static_or_discrete_is_left_alone():
    c = sc.case("box-(0, 'x')@0")
    assert len(_run(c)[1]) == 1
    assert not len(spec.sweep(c.bodies, c.start, np.zeros_like(c.rc), c.kinds, c.polys)[1])
    b = c.bodies.copy()
    b["inv_mass"][c.mover] = 0
    b["inv_inertia"][c.mover] = 0
    assert not len(spec.sweep(b, c.start, c.rc, c.kinds, c.polys)[1])


def test_the_column_between_steps():
    rc = np.array([0, 0.4, 0, 0.25], dtype=F)
    assert spec.spawn(rc, 2).tolist() == [0, F(0.4), 0, 0.25, 0, 0]
    assert spec.remove(rc, [1, 0, 1, 1]).tolist() == [0, 0, 0.25]
    assert spec.set_state(3).tolist() == [0, 0, 0]


# ---- the host check --------------------------------------------------------------------------------------------------------------------------
TRI = [(-2.0, -1.0), (2.0, -1.0), (0.0, 2.0)]


@pytest.mark.parametrize("kind, hx, hy, polygon, inradius", [
    (SHAPE_BOX, 2.0, 0.75, None, 0.75), (SHAPE_BOX, 0.5, 3.0, None, 0.5), (SHAPE_CIRCLE, 1.5, 1.5, None, 1.5), (SHAPE_CAPSULE, 2.0, 0.75, None, 0.75),
    (SHAPE_POLYGON, 2.0, 2.0, TRI, None)])
def test_the_radius_is_held_below_the_inradius(built_lib, kind, hx, hy, polygon, inradius):
    poly = None if polygon is None else ps.polygon(polygon)
    r = spec.inradius(kind, hx, hy, poly)
    if inradius is not None:
        assert r == F(inradius)
    else:
        assert abs(float(r) - 1.0) < 1e-6                                    # the bottom face y = -1 is the nearest
    below = np.nextafter(r, F(0))
    phyx_amd.continuous_check(7, kind, hx, hy, below, polygon)
    phyx_amd.continuous_check(7, kind, hx, hy, 0.0, polygon)
    assert spec.valid(kind, hx, hy, below, poly) and spec.valid(kind, hx, hy, 0.0, poly)
    for rc in (r, np.nextafter(r, F(9)), F(100)):
        assert not spec.valid(kind, hx, hy, rc, poly)
        with pytest.raises(PhxError) as e:
            phyx_amd.continuous_check(7, kind, hx, hy, rc, polygon, what="phx_world_set_continuous")
        assert "phx_world_set_continuous: the core radius %g of body 7 is not below its inradius %g" % (float(rc), float(r)) in str(e.value)


@pytest.mark.parametrize("rc", [-0.25, float("nan"), float("inf"), -float("inf")])
def test_a_radius_is_finite_and_not_negative(built_lib, rc):
    assert not spec.valid(SHAPE_BOX, 1.0, 1.0, rc)
    with pytest.raises(PhxError) as e:
        phyx_amd.continuous_check(3, SHAPE_BOX, 1.0, 1.0, rc)
    assert "the core radius %g of body 3 is not finite and >= 0" % rc in str(e.value)


def test_the_check_refuses_a_polygon_without_its_vertices(built_lib):
    with pytest.raises(PhxError) as e:
        phyx_amd.continuous_check(2, SHAPE_POLYGON, 1.0, 1.0, 0.1)
    assert "body 2 is a polygon and no polygon was given" in str(e.value)


def test_no_device_no_world(built_lib):
    """The four world calls refuse a null handle."""
    L = built_lib
    assert L.phx_world_set_continuous(None, None, None, 0) == -1
    assert L.phx_world_get_continuous(None, None, 0) == -1
    assert L.phx_world_sweep_hits(None, None, 0, None) == -1
    assert L.phx_world_sweep_counts(None, None, None) == -1


# ---- the blob's ninth section ------------------------------------------------------------------------------------------------------------
def _with_column(blob, radii):
    """The blob of a world without the column, given the continuous bodies' section: column bit 8, the section behind the baseline, its
    offset at header byte 112, the new total."""
    import struct
    out = bytearray(blob)
    out[32] |= 8
    struct.pack_into("<Q", out, 40, len(blob) + 16 * len(radii))
    struct.pack_into("<Q", out, 112, len(blob))
    for rc in radii:
        out += struct.pack("<4f", rc, 1.5, -2.5, 0.0)
    return bytes(out)


def test_the_blob_carries_the_column_behind_a_new_bit(built_lib):
    import struct
    import snapshot_cases as cases
    import snapshot_spec
    check = lambda b: built_lib.phx_snapshot_blob_check(b, len(b))      # noqa: E731
    plain = cases.three_body_blob()
    assert check(plain) == 0 and snapshot_spec.check(plain) is None and plain[112:128] == bytes(16)      # a blob written before the bit parses as it did
    good = _with_column(plain, [0.0, 0.4, 0.25])
    assert check(good) == 0
    for name, bad in (("a negative radius", _with_column(plain, [0.0, -0.4, 0.25])), ("a radius that is not finite", _with_column(plain, [0.0, float("inf"), 0.25])),
                      ("the fourth word", good[:len(plain) + 12] + struct.pack("<f", 1.0) + good[len(plain) + 16:]),
                      ("a start that is not finite", good[:len(plain) + 4] + struct.pack("<f", float("nan")) + good[len(plain) + 8:]),
                      ("the offset", good[:112] + struct.pack("<Q", len(plain) + 16) + good[120:]), ("a reserved byte", good[:124] + b"\1" + good[125:]),
                      ("the section without its bit", good[:32] + plain[32:36] + good[36:]), ("the bit without its section", plain[:32] + good[32:36] + plain[36:]),
                      ("a truncated section", good[:-16])):
        assert check(bad) == -1, name
    assert check(plain[:112] + struct.pack("<Q", len(plain)) + plain[120:]) == -1, "an offset at byte 112 without the bit"
