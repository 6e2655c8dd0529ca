"""Round queries (include/phyx_amd.h, QUERIES: phx_world_query_circles / phx_world_cast_circles) without a GPU: the specification
(tests/round_query_spec.py) against the float64 judge (tests/round_query_reference.py, which works by signed distances and shares
nothing with it) on every case of tests/round_query_corpus.py, the specification on hand-built cases with exact expected answers, the
refusals of the entry points and of the Python wrappers, the three symbols in the header, the binding and the library, and
examples/fit.c, which builds and fails loudly without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fit_example
import round_query_corpus as rc
import round_query_spec as spec
from phyx_amd.api import frame_from_angle, rigid_body_dtype
from query_spec import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMBOLS = ("phx_world_query_circles", "phx_world_cast_circles", "phx_world_cast_circles_device")


def _bits(v):
    return np.asarray(v, dtype=F).tobytes()


def _aligned(*boxes, static=(), kinds=None):
    """Axis-aligned bodies (px, py, hx, hy) with the exact frame (1, 0), (0, 1); the AABB is pos -/+ h, exact.  Returns (records, kinds)."""
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
    return b, (None if kinds is None else np.array(kinds, dtype=np.int32))


# ---- the specification against the float64 judge ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in rc.cases()])
def test_spec_against_the_float64_judge(name):
    """Every corpus case, round_query_spec against the judge:
      - every (cast, body) and (circle, body) pair: the rule's verdict is the judge's wherever the clearance exceeds NEAR = 32 u,
        u = 2^-24 * scale; the pairs excused are at most CAP = 0.02 of the case's, by the judge alone;
      - the closest hit: the judge's body, a normal of (0, 0) exactly where the judge has the cast start overlapping, and every
        deviation() measure within the corpus's bounds (16 u; a box's hit 64 u and its normal 128 u: round_query_corpus.BOUNDS says why);
      - the deliberately doubtful casts and circles: excused or right, not counted in the share."""
    c = rc.case(name)
    g = Geometry(c.bodies)
    round_ = c.kinds == rc.CIRCLE
    verdicts = lambda q: spec.cast_body(g, round_, q)[0] & spec.cast_candidate(g, q)      # noqa: E731
    if len(c.casts):
        near, worst = rc.judged("casts", lambda *a: rc.judge_casts(*a, verdicts), c.bodies, c.kinds, c.casts, spec.cast_circles(c.bodies, c.kinds, c.casts))
        assert near.mean() <= rc.CAP, "excluded share %.4f" % near.mean()
        print("%s: %d casts, excluded %.4f of the pairs; worst in u: %s" % (name, len(c.casts), near.mean(), rc.table(worst)))
        rc.assert_bounds(worst, name)
    if len(c.near_casts):
        rc.judge_casts(c.bodies, c.kinds, c.near_casts, spec.cast_circles(c.bodies, c.kinds, c.near_casts), verdicts)
    if len(c.circles):
        near = rc.judge_circles(c.bodies, c.kinds, c.circles, *spec.query_circles(c.bodies, c.kinds, c.circles))
        assert near.mean() <= rc.CAP, "excluded share of the circles' pairs %.4f" % near.mean()
        rc.judge_circles(c.bodies, c.kinds, c.near_circles, *spec.query_circles(c.bodies, c.kinds, c.near_circles))


def test_the_corpus_reaches_every_arm():
    """Over the whole corpus the specification's own answers show every kind of result: no hit, a start inside, the wide box through
    its x face and the tall box through its y face, each corner disc, a circle body; circles that overlap and circles that do not; box
    bodies alone give the same parts but the last."""
    kinds, overlaps, misses = set(), 0, 0
    for c in rc.cases():
        detail = []
        spec.cast_circles(c.bodies, c.kinds, c.casts, detail=detail)
        kinds |= set(detail)
        off, _ = spec.query_circles(c.bodies, c.kinds, c.circles)
        overlaps += int((np.diff(off) > 0).sum())
        misses += int((np.diff(off) == 0).sum())
    assert kinds >= {None, -1, (0, "x"), (1, "y"), 2, 3, 4, 5, 6}, kinds
    assert overlaps > 200 and misses > 100
    c = rc.case("parts")
    bodies, none = rc.boxes_only(c)
    detail = []
    spec.cast_circles(bodies, none, c.casts, detail=detail)
    assert set(detail) >= {(0, "x"), (1, "y"), 2, 3, 4, 5} and 6 not in detail
    exact = [i for i, row in enumerate(c.rows) if isinstance(row[2], str) and row[5] == rc.BOX]
    assert exact, "the exact frames are there: d' has a component of exactly 0 along them"


# ---- the specification on hand-built cases ------------------------------------------------------------------------------------------
def test_spec_tangent_to_a_face_and_to_a_corner_is_overlap():
    b, k = _aligned((0, 0, 1, 1))
    up = float(np.nextafter(F(3), F(4)))
    # a face at distance exactly r; one ulp further; a corner at (3, 4, 5); one ulp further
    off, hits = spec.query_circles(b, k, [[3, 0, 2], [up, 0, 2], [4, 5, 5], [4, float(np.nextafter(F(5), F(6))), 5], [-3, 0.5, 2]])
    assert off.tolist() == [0, 1, 1, 2, 2, 3] and hits.tolist() == [0, 0, 0]      # closed


def test_spec_centre_inside_a_box():
    b, k = _aligned((0, 0, 4, 2))
    off, hits = spec.query_circles(b, k, [[1, -0.5, 1e-3], [3.5, 1.5, 0.25]])
    assert off.tolist() == [0, 1, 2] and hits.tolist() == [0, 0]                  # gx = gy = 0 <= r*r


def test_spec_two_tangent_discs():
    b, k = _aligned((0, 0, 3, 3), kinds=[1])
    up = float(np.nextafter(F(5), F(6)))
    off, hits = spec.query_circles(b, k, [[5, 0, 2], [up, 0, 2], [3, 4, 2], [4.2, 4.2, 2], [3.4, 3.4, 2]])
    # (4.2, 4.2): inside the widened frame square, outside the discs' reach; (3.4, 3.4): 4.81 <= 5
    assert off.tolist() == [0, 1, 1, 2, 2, 3] and hits.tolist() == [0, 0, 0]
    assert spec.query_circles(b, None, [[4.2, 4.2, 2]])[1].tolist() == [0]          # the same record as a box: its corner is 1.7 away


def test_spec_identical_bodies_lowest_index_wins():
    b, k = _aligned((9, 9, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1), kinds=[0, 1, 1])
    assert spec.query_circles(b, k, [[0.5, 0.5, 1]])[1].tolist() == [1, 2]
    assert spec.cast_circles(b, k, [[-6, 0, 1, 1, 0, 10]])["body"].tolist() == [1]


def test_spec_skip_static():
    b, k = _aligned((0, 0, 10, 10), (0, 0, 1, 1), static=(0,))
    assert spec.query_circles(b, k, [[5, 5, 1]])[1].tolist() == [0]
    assert spec.query_circles(b, k, [[5, 5, 1], [0, 0, 1]], skip_static=True)[1].tolist() == [1]
    assert spec.cast_circles(b, k, [[-30, 0, 1, 1, 0, 100]])["body"].tolist() == [0]
    assert spec.cast_circles(b, k, [[-30, 0, 1, 1, 0, 100]], skip_static=True)["body"].tolist() == [1]


def test_spec_nan_aabb_matches_nothing():
    b, k = _aligned((0, 0, 1, 1), (0, 0, 1, 1))
    b[0]["aabb_min"] = (np.nan, 0)
    assert spec.query_circles(b, k, [[0, 0, 1]])[1].tolist() == [1]
    assert spec.cast_circles(b, k, [[-6, 0, 1, 1, 0, 10]])["body"].tolist() == [1]


def test_spec_cast_that_starts_inside():
    for kinds in (None, [1]):
        b, k = _aligned((0, 0, 2, 2), kinds=kinds)
        for c in ([0.5, -0.25, 1, 0, 3, 10], [2.5, 0, 1, -1, 0, 10], [-2.5, 0, 1, -1, 0, 10]):      # inside; overlapping from outside, either way
            h = spec.cast_circles(b, k, [c])[0]
            assert h["body"] == 0 and _bits(h["t"]) == _bits(0.0) and _bits(h["normal"]) == _bits([0.0, 0.0]), (kinds, c)


def test_spec_t_is_never_minus_zero():
    """A cast that starts exactly tangent has tin == 0 or -0 by the arithmetic; t is +0 either way."""
    b, k = _aligned((0, 0, 1, 1), (10, 0, 1, 1), kinds=[0, 1])
    out = spec.cast_circles(b, k, [[-3, 0, 2, 1, 0, 5], [-3, 0, 2, -1, 0, 5], [13, 0, 2, -1, 0, 5], [0, 3, 2, 0, -1, 5]])
    assert out["body"].tolist() == [0, 0, 1, 0]
    assert all(_bits(t) == _bits(0.0) for t in out["t"])


def test_spec_head_on_normal_is_an_exact_negated_copy():
    """A rotated body met head on along its own xv: the wide box's x face, and the normal is -xv bit for bit (a copy, not arithmetic)."""
    fr = frame_from_angle(3.0, 4.0, 0.7)
    b, k = rc.records([(3.0, 4.0, 0.7, 2.0, 1.5, rc.BOX)])
    xv = np.array(tuple(b[0]["xv"]), dtype=F)
    assert _bits(xv) == _bits(fr[2:4])
    o = np.array([3.0, 4.0]) - 20.0 * xv.astype(np.float64)
    detail = []
    h = spec.cast_circles(b, None, [[o[0], o[1], 0.5, xv[0], xv[1], 100]], detail=detail)[0]
    assert h["body"] == 0 and detail == [(0, "x")] and _bits(h["normal"]) == _bits(-xv)
    assert abs(float(h["t"]) - 17.5) < 1e-4
    yv = np.array(tuple(b[0]["yv"]), dtype=F)
    o = np.array([3.0, 4.0]) + 20.0 * yv.astype(np.float64)
    detail = []
    h = spec.cast_circles(b, None, [[o[0], o[1], 0.5, -yv[0], -yv[1], 100]], detail=detail)[0]
    assert detail == [(1, "y")] and _bits(h["normal"]) == _bits(yv)      # from above: +yv, a copy


def test_spec_exact_answers_on_an_aligned_box():
    """The six parts on numbers float32 holds exactly: the box (0, 0) +/- (4, 2), r = 1."""
    b, k = _aligned((0, 0, 4, 2))
    detail = []
    out = spec.cast_circles(b, k, [[-10, 1, 1, 1, 0, 100],         # the wide box's -x face at x = -5: t = 5
                                   [2, 10, 1, 0, -2, 100],         # the tall box's +y face at y = 3: t = 3.5
                                   [4, 10, 1, 0, -1, 100],         # down the line through the corner (4, 2): the corner disc (+,+) at its top, t = 7
                                   [-10, -2, 1, 1, 0, 100],        # along the line through (-4, -2): the disc (-,-) at its left, t = 5
                                   [-10, 3.5, 1, 1, 0, 100],       # past it
                                   [-10, 1, 1, 1, 0, 4.5]],        # stops short
                            detail=detail)
    assert out["body"].tolist() == [0, 0, 0, 0, -1, -1]
    assert out["t"][:4].tolist() == [5.0, 3.5, 7.0, 5.0]
    assert detail == [(0, "x"), (1, "y"), (1, "y"), (0, "x"), None, None]      # (at the arcs' ends the box parts tie with the discs: the first in order)
    assert _bits(out["normal"][0]) == _bits([-1.0, -0.0]) and _bits(out["normal"][1]) == _bits([0.0, 1.0])
    assert _bits(out["normal"][2]) == _bits([0.0, 1.0]) and _bits(out["normal"][3]) == _bits([-1.0, -0.0])
    detail = []
    h = spec.cast_circles(b, k, [[4.6, 10, 1, 0, -1, 100], [-4.6, -10, 1, 0, 1, 100], [-4.6, 10, 1, 0, -1, 100], [4.6, -10, 1, 0, 1, 100]], detail=detail)
    assert detail == [5, 2, 4, 3]                                        # 0.6 beside each corner: its disc, 0.8 above or below it
    assert np.allclose(h["t"], 7.2, atol=1e-5) and np.allclose(np.abs(h["normal"]), [0.6, 0.8], atol=1e-6)
    assert np.sign(h["normal"]).tolist() == [[1, 1], [-1, -1], [-1, 1], [1, -1]]


def test_spec_device_form_rules():
    b, k = _aligned((0, 0, 1, 1))
    bad = [[np.nan, 0, 1], [0, np.inf, 1], [0, 0, 0], [0, 0, -1], [0, 0, np.nan]]
    off, hits = spec.query_circles(b, k, bad + [[0, 0, 1]])
    assert off.tolist() == [0] * 6 + [1] and hits.tolist() == [0]
    ok = [-6, 0, 1]
    casts = [q + [1, 0, 10] for q in bad] + [ok + [0, 0, 10], ok + [-0.0, 0, 10], ok + [1, 0, -1], ok + [1, 0, np.inf], ok + [np.nan, 0, 10], ok + [1, 0, 10]]
    out = spec.cast_circles(b, k, casts)
    assert out["body"].tolist() == [-1] * 10 + [0]
    assert out[:10].tobytes() == spec.cast_circles(b[:0], None, casts[:10]).tobytes()      # body -1, every other field 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_null_handle_is_an_error(built_lib):
    L = built_lib
    q = np.zeros(6, dtype=np.float32)
    out = np.zeros(8, dtype=np.int32)
    total = C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_query_circles(None, vp(q), 1, 0, vp(out), vp(out), 4, C.byref(total)) == -1
    assert L.phx_world_cast_circles(None, vp(q), 1, 0, vp(out)) == -1
    assert L.phx_world_cast_circles_device(None, vp(q), 1, 0, vp(out)) == -1
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


BAD_CIRCLES = {"shape": np.zeros((3, 4), dtype=np.float32), "one row": np.zeros(3, dtype=np.float32), "nan": [[np.nan, 0, 1]], "inf": [[0, np.inf, 1]],
               "beyond float": [[1e39, 0, 1]], "r == 0": [[0, 0, 0]], "r < 0": [[0, 0, -2]], "nan r": [[0, 0, np.nan]],
               "bool": np.zeros((1, 3), dtype=bool), "text": [["a"] * 3]}


@pytest.mark.parametrize("rule", sorted(BAD_CIRCLES))
def test_query_circles_refuses_bad_input(rule):
    with pytest.raises((TypeError, ValueError)):
        _world().query_circles(BAD_CIRCLES[rule])


BAD_CASTS = {"shape": np.zeros((3, 5), dtype=np.float32), "nan c": [[np.nan, 0, 1, 1, 0, 1]], "r == 0": [[0, 0, 0, 1, 0, 1]], "r < 0": [[0, 0, -1, 1, 0, 1]],
             "nan d": [[0, 0, 1, np.nan, 0, 1]], "inf max_t": [[0, 0, 1, 1, 0, np.inf]], "max_t < 0": [[0, 0, 1, 1, 0, -1.0]],
             "d == 0": [[0, 0, 1, 0, 0, 1]], "d == -0": [[0, 0, 1, -0.0, 0, 1]]}


@pytest.mark.parametrize("rule", sorted(BAD_CASTS))
def test_cast_circles_refuses_bad_input(rule):
    with pytest.raises((TypeError, ValueError)):
        _world().cast_circles(BAD_CASTS[rule])


class _Recorder:
    """Answers phx_world_query_circles: PHX_ERR_CAPACITY with the total while the cap is short, then the hits."""

    def __init__(self, counts):
        self.counts, self.caps, self.flags = counts, [], []

    def phx_world_query_circles(self, h, circles, count, flags, offsets, hits, cap, total):
        self.caps.append(cap); self.flags.append(flags)
        off = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_int32)), shape=(count + 1,))
        off[:] = np.concatenate([[0], np.cumsum(self.counts)])
        C.cast(total, C.POINTER(C.c_int64))[0] = int(off[-1])
        if off[-1] > cap:
            return -4
        out = np.ctypeslib.as_array(C.cast(hits, C.POINTER(C.c_int32)), shape=(cap,))
        out[:off[-1]] = np.arange(off[-1])
        return 0


def test_query_circles_retries_once_with_the_reported_total():
    rec = _Recorder([3000, 0, 2])
    offsets, hits = _world(rec).query_circles([[0, 0, 1]] * 3, skip_static=True)
    assert rec.caps == [1024, 3002] and rec.flags == [1, 1]
    assert offsets.tolist() == [0, 3000, 3000, 3002] and hits.tolist() == list(range(3002))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_three_symbols(built_lib):
    from phyx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "phyx_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "phyx_amd", "libphyx_amd.so")], text=True)
    for name in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert decl, "%s is not declared in include/phyx_amd.h" % name
        assert name in _lib.declared_symbols() and hasattr(built_lib, name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), "%s is not exported" % name
        fn = getattr(built_lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(decl.group(1).split(",")), name


# ---- the example --------------------------------------------------------------------------------------------------------------------
def test_fit_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = fit_example.build(tmp_path)
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        return                                                          # (its run is the gpu test's)
    r = subprocess.run([exe, "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
