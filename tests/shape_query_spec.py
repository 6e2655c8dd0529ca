"""The World's shape queries stated in numpy (include/phyx_amd.h, QUERIES: oriented boxes and box casts): the specification the device is
held to, byte for byte.

Every formula is the header's, one float32 operation at a time, over the 128-byte records of World.bodies().  Geometry, the one-axis
slab and the two-axis ray test are those of tests/query_spec.py.  The device forms' rule is folded in: a query with a non-finite
component or a half extent <= 0, a cast with max_t < 0 or a zero direction matches nothing (the host forms refuse such input before it
gets here)."""
import numpy as np

from phyx_amd.api import shape_hit_dtype
from query_spec import F, Geometry, _slab, ray_test


def box_ok(q):
    q = np.asarray(q, dtype=F)
    return bool(np.isfinite(q).all() and q[6] > 0 and q[7] > 0)


def cast_ok(c):
    c = np.asarray(c, dtype=F)
    return bool(box_ok(c[:8]) and np.isfinite(c[8:]).all() and c[10] >= 0 and (c[8] != 0 or c[9] != 0))


def extents(q):
    """ex = |X.x|*H.x + |Y.x|*H.y, ey = |X.y|*H.x + |Y.y|*H.y"""
    px, py, xx, xy, yx, yy, hx, hy = (F(v) for v in q)
    return np.abs(xx) * hx + np.abs(yx) * hy, np.abs(xy) * hx + np.abs(yy) * hy


def axes(g, q):
    """The four axes in order: X, Y (the query's, scalars), xv, yv (each body's)."""
    px, py, xx, xy, yx, yy, hx, hy = (F(v) for v in q)
    return [(xx, xy), (yx, yy), (g.xvx, g.xvy), (g.yvx, g.yvy)]


def axis(g, q, ax, ay):
    """(s, R) of every body on the axis A = (ax, ay): the same expression for all four axes."""
    px, py, xx, xy, yx, yy, hx, hy = (F(v) for v in q)
    cx = px - g.px
    cy = py - g.py
    s = cx * ax + cy * ay
    rq = np.abs(xx * ax + xy * ay) * hx + np.abs(yx * ax + yy * ay) * hy
    rb = np.abs(g.xvx * ax + g.xvy * ay) * g.hx + np.abs(g.yvx * ax + g.yvy * ay) * g.hy
    return s, rq + rb


def box_overlap(g, q):
    px, py = F(q[0]), F(q[1])
    ex, ey = extents(q)
    hit = (g.lox - ex <= px) & (g.hix + ex >= px) & (g.loy - ey <= py) & (g.hiy + ey >= py)
    for ax, ay in axes(g, q):
        s, R = axis(g, q, ax, ay)
        hit &= np.abs(s) <= R
    return hit


def cast_candidate(g, c):
    px, py, dx, dy, max_t = F(c[0]), F(c[1]), F(c[8]), F(c[9]), F(c[10])
    ex, ey = extents(c[:8])
    ordered = (g.lox <= g.hix) & (g.loy <= g.hiy)
    hit, _, _ = ray_test(px, py, dx, dy, g.lox - ex, g.loy - ey, g.hix + ex, g.hiy + ey, max_t)
    return ordered & hit


def cast_box(g, c):
    """The four slabs against every body: (pass, tin, the entering axis 0..3, v on it)."""
    dx, dy, max_t = F(c[8]), F(c[9]), F(c[10])
    ok = np.ones(g.n, dtype=bool)
    tin = tout = enter = ventered = None
    for k, (ax, ay) in enumerate(axes(g, c[:8])):
        s, R = axis(g, c[:8], ax, ay)
        v = np.broadcast_to(dx * ax + dy * ay, (g.n,))
        okk, t0, t1 = _slab(s, v, -R, R)
        ok &= okk
        if k == 0:
            tin, tout, enter, ventered = t0, t1, np.zeros(g.n, dtype=np.int32), v
        else:
            later = t0 > tin                                            # (strictly: the first axis that attains tin stays)
            tin = np.where(later, t0, tin).astype(F)
            enter = np.where(later, k, enter)
            ventered = np.where(later, v, ventered).astype(F)
            tout = np.where(t1 < tout, t1, tout).astype(F)
    return ok & (tin <= tout) & (tout >= 0) & (tin <= max_t), tin, enter, ventered


def query_boxes(bodies, boxes, skip_static=False):
    g = Geometry(bodies)
    bs = np.asarray(boxes, dtype=F).reshape(-1, 8)
    elig = g.eligible(skip_static)
    segs = []
    for q in bs:
        if not box_ok(q) or not g.n:
            segs.append(np.zeros(0, dtype=np.int32))
            continue
        segs.append(np.flatnonzero(elig & box_overlap(g, q)).astype(np.int32))
    offsets = np.zeros(len(bs) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in segs]) if segs else []
    hits = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int32)
    return offsets, hits.astype(np.int32)


def cast_boxes(bodies, casts, skip_static=False, detail=None):
    """`detail` (a list) receives per cast the entering axis of the winner: 0..3, -1 for a start inside, None for no hit."""
    g = Geometry(bodies)
    cs = np.asarray(casts, dtype=F).reshape(-1, 11)
    out = np.zeros(len(cs), dtype=shape_hit_dtype)
    out["body"] = -1
    elig = g.eligible(skip_static)
    for q, c in enumerate(cs):
        kind = None
        if cast_ok(c) and g.n:
            hit, tin, enter, v = cast_box(g, c)
            hit &= elig & cast_candidate(g, c)
            if hit.any():
                t = np.where(tin > 0, tin, F(0)).astype(F)
                tmin = t[hit].min()
                b = int(np.flatnonzero(hit & (t == tmin))[0])           # smallest t, then the lowest index
                out["body"][q] = b
                out["t"][q] = tmin
                kind = -1
                if not tin[b] < 0:
                    kind = int(enter[b])
                    ax, ay = axes(g, c[:8])[kind]
                    n = (F(ax), F(ay)) if kind < 2 else (ax[b], ay[b])
                    out["normal"][q] = (-n[0], -n[1]) if v[b] > 0 else n
        if detail is not None:
            detail.append(kind)
    return out
