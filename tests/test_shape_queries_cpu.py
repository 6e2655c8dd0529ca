"""Shape queries (include/phyx_amd.h, QUERIES: phx_world_query_boxes / phx_world_cast_boxes) without a GPU: the specification
(tests/shape_query_spec.py) against a float64 separating-axis test and a float64 bisection that share no code with it, on the 0 .. 100
field and on the same field moved out to (3000, -7000) and (10^5, 10^5), the specification
on hand-built boundary cases, the refusals of the entry points and of the Python wrappers, and examples/place.c, which builds and fails
loudly without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shape_query_spec as spec
from query_spec import Geometry
from phyx_amd.api import box_from_angle, frame_from_angle, rigid_body_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MARGIN = 1e-3           # pairs with a float64 axis gap this close to zero may be left out (at coordinates 0 .. 100) ...
CAP = 0.02              # ... and at most this share of the pairs
SHIFTS = ((3000.0, -7000.0), (1e5, 1e5))      # the 0 .. 100 field moved out to where the project's worlds reach


def _margin(shift):
    """MARGIN widened by the coordinate's ulp.  The rules work on differences of nearby floats (c = P - pos, exact or rounded at the
    size of c), so moving the field adds nothing to what they lose but for the AABB conjunct and the candidate test, which round
    a.min - e, a.max + e and the AABB itself at the size of the coordinates: two roundings, 4 ulp with a factor 2 to spare.  (MARGIN
    times the ratio of the ulps, 1.02 at 10^5, would by the float64 check alone exclude 0.11 of the overlap pairs and 0.23 of the casts
    of this field, against CAP; this margin is the narrower one and asks more.)"""
    reach = 100.0 + max(abs(shift[0]), abs(shift[1]))
    return MARGIN + 4.0 * float(np.spacing(F(reach)) - np.spacing(F(100.0)))


def _shifted(rows, shift):
    """The rows moved by `shift`, their positions rounded to float32 as the records and the query boxes will hold them: the float64
    check and the specification then start from the same floats."""
    out = np.array(rows, dtype=np.float64)
    out[:, 0:2] = (out[:, 0:2] + np.asarray(shift)).astype(F)
    return out


def _records(rows, static=()):
    """Bodies (px, py, angle, hx, hy) as add_body frames them; the AABB is pos -/+ (|xv|*h.x + |yv|*h.y), in float32."""
    b = np.zeros(len(rows), dtype=rigid_body_dtype)
    for i, (px, py, ang, hx, hy) in enumerate(rows):
        fr = frame_from_angle(px, py, ang)
        b[i]["index"] = i
        b[i]["pos"] = b[i]["geom_pos"] = tuple(fr[0:2])
        b[i]["xv"] = b[i]["geom_xv"] = tuple(fr[2:4])
        b[i]["yv"] = b[i]["geom_yv"] = tuple(fr[4:6])
        b[i]["geom_size"] = (hx, hy)
        ex = np.abs(fr[2]) * F(hx) + np.abs(fr[4]) * F(hy)
        ey = np.abs(fr[3]) * F(hx) + np.abs(fr[5]) * F(hy)
        b[i]["aabb_min"] = (fr[0] - ex, fr[1] - ey)
        b[i]["aabb_max"] = (fr[0] + ex, fr[1] + ey)
        b[i]["inv_mass"], b[i]["inv_inertia"] = (0, 0) if i in static else (1, 1)
    return b


def _aligned(*boxes, static=()):
    """Axis-aligned bodies (px, py, hx, hy) with the exact frame (1, 0), (0, 1); the AABB is pos -/+ h, exact."""
    b = np.zeros(len(boxes), dtype=rigid_body_dtype)
    for i, (px, py, hx, hy) in enumerate(boxes):
        b[i]["index"] = i
        b[i]["pos"] = b[i]["geom_pos"] = (px, py)
        b[i]["xv"] = b[i]["geom_xv"] = (1, 0)
        b[i]["yv"] = b[i]["geom_yv"] = (0, 1)
        b[i]["geom_size"] = (hx, hy)
        b[i]["aabb_min"] = (F(px) - F(hx), F(py) - F(hy))
        b[i]["aabb_max"] = (F(px) + F(hx), F(py) + F(hy))
        b[i]["inv_mass"], b[i]["inv_inertia"] = (0, 0) if i in static else (1, 1)
    return b


def _box(px, py, hx, hy):
    """An axis-aligned query box with the exact frame."""
    return [px, py, 1, 0, 0, 1, hx, hy]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


# ---- the independent check: float64, from the angles, by projecting corners ---------------------------------------------------------
def _corners64(rows):
    """(N, 4, 2) corners and (N, 2, 2) unit edge directions of boxes (px, py, angle, hx, hy), in float64."""
    r = np.asarray(rows, dtype=np.float64)
    c, s = np.cos(r[:, 2]), np.sin(r[:, 2])
    u = np.stack([c, s], axis=1)
    v = np.stack([-s, c], axis=1)
    sign = np.array([[1, 1], [1, -1], [-1, -1], [-1, 1]], dtype=np.float64)
    pts = r[:, None, 0:2] + sign[None, :, 0:1] * r[:, None, 3:4] * u[:, None, :] + sign[None, :, 1:2] * r[:, None, 4:5] * v[:, None, :]
    return pts, np.stack([u, v], axis=1)


def _intervals64(qpts, qdir, bpts, bdir, d=None):
    """The projection intervals of every query box and every body on the four edge directions, (Q, N, 4) each: (query min, query max,
    body min, body max), and the speed of the query along each direction when it moves by d (Q, 2)."""
    q, n = len(qpts), len(bpts)
    axes = np.concatenate([np.broadcast_to(qdir[:, None, :, :], (q, n, 2, 2)), np.broadcast_to(bdir[None, :, :, :], (q, n, 2, 2))], axis=2)
    pq = np.einsum("qci,qnai->qnac", qpts, axes)
    pb = np.einsum("nci,qnai->qnac", bpts, axes)
    speed = np.einsum("qi,qnai->qna", d, axes) if d is not None else 0.0
    return pq.min(axis=3), pq.max(axis=3), pb.min(axis=3), pb.max(axis=3), speed


def _gaps64(iv, t=None):
    """(Q, N, 4) interval gaps on the four edge directions, the query moved for the time t (Q, N)."""
    qmin, qmax, bmin, bmax, speed = iv
    move = 0.0 if t is None else t[:, :, None] * speed
    return np.maximum(bmin - (qmax + move), (qmin + move) - bmax)


def _random_rows(rng, n):
    return np.stack([rng.uniform(0, 100, n), rng.uniform(0, 100, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0.5, 20, n), rng.uniform(0.5, 20, n)], axis=1)


NQ, NB = 200, 110                                                      # 22 000 pairs


def _overlap_against_float64(shift):
    rng = np.random.default_rng(20240)
    brow, qrow = _shifted(_random_rows(rng, NB), shift), _shifted(_random_rows(rng, NQ), shift)
    margin = _margin(shift)
    g = Geometry(_records(brow))
    gaps = _gaps64(_intervals64(*_corners64(qrow), *_corners64(brow)))
    want = (gaps <= 0).all(axis=2)
    near = np.abs(gaps).min(axis=2) < margin
    assert NQ * NB >= 20000 and near.mean() <= CAP, "excluded share %.4f" % near.mean()
    got = np.stack([spec.box_overlap(g, box_from_angle(*q)) for q in qrow])
    assert want.sum() > 1000 and (~want).sum() > 1000
    assert (got == want)[~near].all(), "%d of %d pairs disagree" % ((got != want)[~near].sum(), (~near).sum())


def test_spec_overlap_agrees_with_a_float64_separating_axis_test():
    _overlap_against_float64((0.0, 0.0))


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: "%g,%g" % s)
def test_spec_overlap_agrees_with_float64_on_a_field_far_from_the_origin(shift):
    _overlap_against_float64(shift)


def _cast_t_against_float64(shift):
    rng = np.random.default_rng(20241)
    brow, qrow = _shifted(_random_rows(rng, NB), shift), _shifted(_random_rows(rng, NQ), shift)
    margin = _margin(shift)
    ang = rng.uniform(0, 2 * np.pi, NQ)
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(0.5, 3.0, (NQ, 1))
    max_t = rng.uniform(5.0, 60.0, NQ)
    casts = np.stack([np.concatenate([box_from_angle(*q), dd.astype(F), [F(m)]]) for q, dd, m in zip(qrow, d, max_t)]).astype(F)
    g = Geometry(_records(brow))
    qpts, qdir = _corners64(qrow)
    bpts, bdir = _corners64(brow)
    d64, m64 = casts[:, 8:10].astype(np.float64), casts[:, 10].astype(np.float64)

    iv = _intervals64(qpts, qdir, bpts, bdir, d64)

    def worst(t):                                                      # the largest axis gap at time t (Q, N): convex in t; overlap iff <= 0
        return _gaps64(iv, t).max(axis=2)

    def closest_to_zero(t):
        return np.abs(_gaps64(iv, t)).min(axis=2)

    zero = np.zeros((NQ, NB))
    end = np.broadcast_to(m64[:, None], (NQ, NB)).copy()
    lo, hi = zero.copy(), end.copy()
    for _ in range(64):                                                # the minimiser of the convex `worst` over [0, max_t]
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        left = worst(a) <= worst(b)
        hi = np.where(left, b, hi)
        lo = np.where(left, lo, a)
    tmin = 0.5 * (lo + hi)
    inside0, reaches = worst(zero) <= 0, worst(tmin) <= 0
    want_hit = inside0 | reaches
    lo, hi = zero.copy(), tmin.copy()                                  # `worst` falls on [0, tmin]: bisect the predicate there
    for _ in range(44):
        mid = 0.5 * (lo + hi)
        over = worst(mid) <= 0
        hi = np.where(over, mid, hi)
        lo = np.where(over, lo, mid)
    want_t = np.where(inside0, 0.0, hi)
    near = (closest_to_zero(zero) < margin) | (closest_to_zero(tmin) < margin) | (closest_to_zero(end) < margin)
    near |= want_hit & ~inside0 & (np.abs(want_t - end) < margin)
    assert near.mean() <= CAP, "excluded share %.4f" % near.mean()
    got_hit, got_t = np.zeros((NQ, NB), dtype=bool), np.zeros((NQ, NB))
    for q, c in enumerate(casts):
        hit, tin, _, _ = spec.cast_box(g, c)
        got_hit[q] = hit & spec.cast_candidate(g, c)
        got_t[q] = np.where(tin > 0, tin, 0)
    keep = ~near
    assert (want_hit & keep).sum() > 500 and (~want_hit & keep).sum() > 500
    assert (got_hit == want_hit)[keep].all(), "%d pairs disagree on the hit" % (got_hit != want_hit)[keep].sum()
    both = keep & want_hit
    err = np.abs(got_t - want_t)[both]
    assert (err <= 1e-3 * np.abs(want_t[both]) + margin).all(), "largest t error %g" % err.max()


def test_spec_cast_t_agrees_with_a_float64_bisection():
    _cast_t_against_float64((0.0, 0.0))


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: "%g,%g" % s)
def test_spec_cast_t_agrees_with_float64_on_a_field_far_from_the_origin(shift):
    _cast_t_against_float64(shift)


# ---- the specification on hand-built cases ------------------------------------------------------------------------------------------
def test_spec_edge_and_corner_touch_are_overlap():
    b = _aligned((0, 0, 1, 1))
    up = float(np.nextafter(F(2), F(3)))
    off, hits = spec.query_boxes(b, [_box(2, 0, 1, 1), _box(up, 0, 1, 1), _box(2, 2, 1, 1), _box(2, up, 1, 1), _box(-2, -2, 1, 1)])
    assert off.tolist() == [0, 1, 1, 2, 2, 3] and hits.tolist() == [0, 0, 0]      # closed: |s| == R on an edge and at a corner


def test_spec_query_box_identical_to_a_body():
    rows = [(3.0, 4.0, 0.7, 2.0, 1.5), (40.0, 4.0, 0.2, 2.0, 1.5)]
    b = _records(rows)
    q = box_from_angle(*rows[0])
    assert spec.query_boxes(b, [q])[1].tolist() == [0]
    h = spec.cast_boxes(b, [np.concatenate([q, [1, 0, 100]])])[0]
    assert h["body"] == 0 and _bits(h["t"]) == _bits(0.0) and _bits(h["normal"]) == _bits([0.0, 0.0])


def test_spec_identical_bodies_lowest_index_wins():
    b = _aligned((9, 9, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1))
    assert spec.query_boxes(b, [_box(0.5, 0.5, 1, 1)])[1].tolist() == [1, 2]
    assert spec.cast_boxes(b, [_box(-6, 0, 1, 1) + [1, 0, 10]])["body"].tolist() == [1]


def test_spec_cast_that_starts_overlapping():
    h = spec.cast_boxes(_aligned((0, 0, 1, 1)), [_box(0.5, -0.25, 1, 1) + [0, 3, 10]])[0]
    assert h["body"] == 0 and _bits(h["t"]) == _bits(0.0) and _bits(h["normal"]) == _bits([0.0, 0.0])


def test_spec_cast_parallel_to_a_face_at_the_touching_distance():
    b = _aligned((0, 0, 1, 1))
    kinds = []
    h = spec.cast_boxes(b, [_box(-10, 2, 1, 1) + [1, 0, 100]], detail=kinds)[0]      # |s| == R on y, v == 0 there: the slab is all of t
    assert h["body"] == 0 and h["t"] == 8 and kinds == [0]                           # X and xv both enter at 8: the first in order
    assert _bits(h["normal"]) == _bits([-1.0, -0.0])                                 # -X: against the motion
    assert spec.cast_boxes(b, [_box(-10, float(np.nextafter(F(2), F(3))), 1, 1) + [1, 0, 100]])[0]["body"] == -1


def test_spec_cast_stops_short_at_max_t():
    b = _aligned((0, 0, 1, 1))
    assert spec.cast_boxes(b, [_box(-10, 0, 1, 1) + [1, 0, 7.5]])[0]["body"] == -1
    h = spec.cast_boxes(b, [_box(-10, 0, 1, 1) + [1, 0, 8]])[0]                      # closed at max_t
    assert h["body"] == 0 and h["t"] == 8


def test_spec_zero_component_of_d_in_the_body_frame():
    b = _aligned((0, 0, 2, 1))
    kinds = []
    h = spec.cast_boxes(b, [_box(0.5, 10, 1, 1) + [0, -3, 100]], detail=kinds)[0]    # v == 0 on X and xv; Y enters first
    assert h["body"] == 0 and h["t"] == F(8) / F(3) and kinds == [1]
    assert _bits(h["normal"]) == _bits([0.0, 1.0])                                   # +Y: v < 0
    assert spec.cast_boxes(b, [_box(3.5, 10, 1, 1) + [0, -3, 100]])[0]["body"] == -1  # outside the x slab: empty for every t


def test_spec_entry_through_a_body_axis():
    """A rotated body: the tilted face of the body is what the box meets, so the entering axis is one of the body's."""
    b = _records([(0.0, 0.0, np.pi / 4, 4.0, 4.0)])
    kinds = []
    h = spec.cast_boxes(b, [_box(-20, -20, 0.1, 0.1) + [1, 1, 100]], detail=kinds)[0]
    assert h["body"] == 0 and kinds == [2]                                           # the face whose normal is xv = (cos, sin)(pi / 4)
    xv = np.array(tuple(b[0]["xv"]), dtype=F)
    assert _bits(h["normal"]) == _bits(-xv)                                          # an exact negation: against the motion


def test_spec_skip_static():
    b = _aligned((0, 0, 10, 10), (0, 0, 1, 1), static=(0,))
    assert spec.query_boxes(b, [_box(5, 5, 1, 1)])[1].tolist() == [0]
    assert spec.query_boxes(b, [_box(5, 5, 1, 1), _box(0, 0, 1, 1)], skip_static=True)[1].tolist() == [1]
    assert spec.cast_boxes(b, [_box(-30, 0, 1, 1) + [1, 0, 100]])["body"].tolist() == [0]
    assert spec.cast_boxes(b, [_box(-30, 0, 1, 1) + [1, 0, 100]], skip_static=True)["body"].tolist() == [1]


def test_spec_nan_aabb_matches_nothing():
    b = _aligned((0, 0, 1, 1), (0, 0, 1, 1))
    b[0]["aabb_min"] = (np.nan, 0)
    assert spec.query_boxes(b, [_box(0, 0, 1, 1)])[1].tolist() == [1]
    assert spec.cast_boxes(b, [_box(-6, 0, 1, 1) + [1, 0, 10]])["body"].tolist() == [1]


def test_spec_device_form_rules():
    b = _aligned((0, 0, 1, 1))
    bad = [_box(np.nan, 0, 1, 1), _box(0, 0, np.inf, 1), _box(0, 0, 0, 1), _box(0, 0, 1, -1), [0, 0, 1, np.nan, 0, 1, 1, 1]]
    off, hits = spec.query_boxes(b, bad + [_box(0, 0, 1, 1)])
    assert off.tolist() == [0] * 6 + [1] and hits.tolist() == [0]
    ok = _box(-6, 0, 1, 1)
    casts = [q + [1, 0, 10] for q in bad] + [ok + [0, 0, 10], ok + [-0.0, 0, 10], ok + [1, 0, -1], ok + [1, 0, np.inf], ok + [np.nan, 0, 10], ok + [1, 0, 10]]
    out = spec.cast_boxes(b, casts)
    assert out["body"].tolist() == [-1] * 10 + [0]
    assert out[:10].tobytes() == spec.cast_boxes(b[:0], casts[:10]).tobytes()      # body -1, every other field 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_null_handle_is_an_error(built_lib):
    L = built_lib
    q = np.zeros(11, dtype=np.float32)
    out = np.zeros(8, dtype=np.int32)
    total = C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_query_boxes(None, vp(q), 1, 0, vp(out), vp(out), 4, C.byref(total)) == -1
    assert L.phx_world_cast_boxes(None, vp(q), 1, 0, vp(out)) == -1
    assert L.phx_world_cast_boxes_device(None, vp(q), 1, 0, vp(out)) == -1
    assert b"null handle" in L.phx_last_error()


class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world(lib=None):
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = lib if lib is not None else _NoC(), None
    return w


BAD_BOXES = {"shape": np.zeros((3, 7), dtype=np.float32), "one row": np.zeros(8, dtype=np.float32), "nan": [_box(np.nan, 0, 1, 1)],
             "inf": [_box(0, np.inf, 1, 1)], "beyond float": [_box(1e39, 0, 1, 1)], "h.x == 0": [_box(0, 0, 0, 1)], "h.y < 0": [_box(0, 0, 1, -2)],
             "bool": np.zeros((1, 8), dtype=bool), "text": [["a"] * 8]}


@pytest.mark.parametrize("rule", sorted(BAD_BOXES))
def test_query_boxes_refuses_bad_input(rule):
    with pytest.raises((TypeError, ValueError)):
        _world().query_boxes(BAD_BOXES[rule])


BAD_CASTS = {"shape": np.zeros((3, 8), dtype=np.float32), "nan box": [_box(np.nan, 0, 1, 1) + [1, 0, 1]], "h.x == 0": [_box(0, 0, 0, 1) + [1, 0, 1]],
             "h.y < 0": [_box(0, 0, 1, -1) + [1, 0, 1]], "nan d": [_box(0, 0, 1, 1) + [np.nan, 0, 1]], "inf max_t": [_box(0, 0, 1, 1) + [1, 0, np.inf]],
             "max_t < 0": [_box(0, 0, 1, 1) + [1, 0, -1.0]], "d == 0": [_box(0, 0, 1, 1) + [0, 0, 1]], "d == -0": [_box(0, 0, 1, 1) + [-0.0, 0, 1]]}


@pytest.mark.parametrize("rule", sorted(BAD_CASTS))
def test_cast_boxes_refuses_bad_input(rule):
    with pytest.raises((TypeError, ValueError)):
        _world().cast_boxes(BAD_CASTS[rule])


class _Recorder:
    """Answers phx_world_query_boxes: PHX_ERR_CAPACITY with the total while the cap is short, then the hits."""

    def __init__(self, counts):
        self.counts, self.caps, self.flags = counts, [], []

    def phx_world_query_boxes(self, h, boxes, count, flags, offsets, hits, cap, total):
        self.caps.append(cap); self.flags.append(flags)
        off = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_int32)), shape=(count + 1,))
        off[:] = np.concatenate([[0], np.cumsum(self.counts)])
        C.cast(total, C.POINTER(C.c_int64))[0] = int(off[-1])
        if off[-1] > cap:
            return -4
        out = np.ctypeslib.as_array(C.cast(hits, C.POINTER(C.c_int32)), shape=(cap,))
        out[:off[-1]] = np.arange(off[-1])
        return 0


def test_query_boxes_retries_once_with_the_reported_total():
    rec = _Recorder([3000, 0, 2])
    offsets, hits = _world(rec).query_boxes([_box(0, 0, 1, 1)] * 3, skip_static=True)
    assert rec.caps == [1024, 3002] and rec.flags == [1, 1]
    assert offsets.tolist() == [0, 3000, 3000, 3002] and hits.tolist() == list(range(3002))


def test_box_from_angle_is_the_frame_add_body_builds():
    q = box_from_angle(3.0, -2.0, 0.3, 5.0, 4.0)
    assert q.dtype == np.float32 and q.shape == (8,)
    assert q[:6].tobytes() == frame_from_angle(3.0, -2.0, 0.3).tobytes() and q[6:].tolist() == [5.0, 4.0]


def test_place_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = str(tmp_path / "place")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "place.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        return                                                          # (its run is the gpu test's)
    r = subprocess.run([exe, "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
