"""The World's round queries stated in numpy (include/phyx_amd.h, QUERIES: query circles and circle casts): the specification the
device is held to, byte for byte.

Every formula is the header's, one float32 operation at a time, over the 128-byte records of World.bodies() and the kinds of
World.shapes() (None: a world of boxes).  Geometry, the one-axis slab and the two-axis ray test are those of tests/query_spec.py; the
ray/disc rule is stated here with the origin already taken relative to the centre, as the header's circle cast uses it.  The device
forms' rule is folded in: a query with a non-finite component or a radius <= 0, a cast with max_t < 0 or a zero direction matches
nothing (the host forms refuse such input before it gets here)."""
import numpy as np

from phyx_amd.api import shape_hit_dtype
from query_spec import F, Geometry, ray_test

CIRCLE = 1
WIDE, TALL, CORNERS, BODY = 0, 1, (2, 3, 4, 5), 6      # the parts of a cast: the two boxes, the corner discs (-,-) (+,-) (-,+) (+,+), a circle body


def _round(g, kinds):
    return np.zeros(g.n, dtype=bool) if kinds is None else np.asarray(kinds) == CIRCLE


def circle_ok(c):
    c = np.asarray(c, dtype=F)
    return bool(np.isfinite(c).all() and c[2] > 0)


def cast_ok(c):
    c = np.asarray(c, dtype=F)
    return bool(circle_ok(c[:3]) and np.isfinite(c[3:]).all() and c[5] >= 0 and (c[3] != 0 or c[4] != 0))


def near(g, cx, cy, r):
    """a.min.x - r <= c.x && a.max.x + r >= c.x && a.min.y - r <= c.y && a.max.y + r >= c.y"""
    return (g.lox - r <= cx) & (g.hix + r >= cx) & (g.loy - r <= cy) & (g.hiy + r >= cy)


def overlap(g, round_, c):
    cx, cy, r = (F(v) for v in c)
    with np.errstate(all="ignore"):
        ex = cx - g.px
        ey = cy - g.py
        R = r + g.hx
        disc = ex * ex + ey * ey <= R * R
        u = ex * g.xvx + ey * g.xvy
        v = ex * g.yvx + ey * g.yvy
        qu = np.where(u < -g.hx, -g.hx, np.where(u > g.hx, g.hx, u)).astype(F)
        qv = np.where(v < -g.hy, -g.hy, np.where(v > g.hy, g.hy, v)).astype(F)
        gx = u - qu
        gy = v - qv
        box = gx * gx + gy * gy <= r * r
    return near(g, cx, cy, r) & np.where(round_, disc, box)


def ray_disc(rx, ry, dx, dy, max_t, rad):
    """The ray/disc rule (the closest-approach form) with the origin relative to the centre: (pass, tin, nx, ny)."""
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy
        b = rx * dx + ry * dy
        tc = -b / a
        ex = rx + tc * dx
        ey = ry + tc * dy
        h2 = rad * rad - (ex * ex + ey * ey)
        s = np.sqrt(h2 / a)
        tin = (tc - s).astype(F)
        tout = (tc + s).astype(F)
        hit = (h2 >= 0) & (tin <= tout) & (tout >= 0) & (tin <= max_t)
        return hit, tin, (ex - s * dx).astype(F), (ey - s * dy).astype(F)


def cast_candidate(g, c):
    cx, cy, r, dx, dy, max_t = (F(v) for v in c)
    ordered = (g.lox <= g.hix) & (g.loy <= g.hiy)
    hit, _, _ = ray_test(cx, cy, dx, dy, g.lox - r, g.loy - r, g.hix + r, g.hiy + r, max_t)
    return ordered & hit


def cast_body(g, round_, c):
    """The cast against every body's own shape: (pass, tin, part, o'.x, o'.y, d'.x, d'.y, nx, ny)."""
    cx, cy, r, dx, dy, max_t = (F(v) for v in c)
    with np.errstate(all="ignore"):
        rx = cx - g.px
        ry = cy - g.py
        chit, ctin, cnx, cny = ray_disc(rx, ry, dx, dy, max_t, r + g.hx)
        ox = rx * g.xvx + ry * g.xvy
        oy = rx * g.yvx + ry * g.yvy
        dxp = dx * g.xvx + dy * g.xvy
        dyp = dx * g.yvx + dy * g.yvy
        wx = g.hx + r
        wy = g.hy + r
        hit, tin, _ = ray_test(ox, oy, dxp, dyp, -wx, -g.hy, wx, g.hy, max_t)
        tin = np.where(hit, tin, F(0)).astype(F)
        part = np.zeros(g.n, dtype=np.int32)
        nx = np.zeros(g.n, dtype=F)
        ny = np.zeros(g.n, dtype=F)
        ok, t, _ = ray_test(ox, oy, dxp, dyp, -g.hx, -wy, g.hx, wy, max_t)
        better = ok & (~hit | (t < tin))
        tin, part, hit = np.where(better, t, tin).astype(F), np.where(better, TALL, part), hit | ok
        for k, (sx, sy) in zip(CORNERS, ((-1, -1), (1, -1), (-1, 1), (1, 1))):
            kx = g.hx if sx > 0 else -g.hx
            ky = g.hy if sy > 0 else -g.hy
            ok, t, px, py = ray_disc(ox - kx, oy - ky, dxp, dyp, max_t, r)
            better = ok & (~hit | (t < tin))
            tin, part, hit = np.where(better, t, tin).astype(F), np.where(better, k, part), hit | ok
            nx, ny = np.where(better, px, nx).astype(F), np.where(better, py, ny).astype(F)
    return (np.where(round_, chit, hit), np.where(round_, ctin, tin).astype(F), np.where(round_, BODY, part), ox, oy, dxp, dyp,
            np.where(round_, cnx, nx).astype(F), np.where(round_, cny, ny).astype(F))


def query_circles(bodies, kinds, circles, skip_static=False):
    g = Geometry(bodies)
    round_ = _round(g, kinds)
    cs = np.asarray(circles, dtype=F).reshape(-1, 3)
    elig = g.eligible(skip_static)
    segs = []
    for c in cs:
        if not circle_ok(c) or not g.n:
            segs.append(np.zeros(0, dtype=np.int32))
            continue
        segs.append(np.flatnonzero(elig & overlap(g, round_, c)).astype(np.int32))
    offsets = np.zeros(len(cs) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in segs]) if segs else []
    hits = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int32)
    return offsets, hits.astype(np.int32)


def cast_circles(bodies, kinds, casts, skip_static=False, detail=None):
    """`detail` (a list) receives per cast the winning part: 0 / 1 with the face's axis as (part, "x" | "y"), 2..5, 6 (a circle body), -1
    for a start inside, None for no hit."""
    g = Geometry(bodies)
    round_ = _round(g, kinds)
    cs = np.asarray(casts, dtype=F).reshape(-1, 6)
    out = np.zeros(len(cs), dtype=shape_hit_dtype)
    out["body"] = -1
    elig = g.eligible(skip_static)
    for q, c in enumerate(cs):
        kind = None
        if cast_ok(c) and g.n:
            hit, tin, part, ox, oy, dxp, dyp, nx, ny = cast_body(g, round_, c)
            hit = hit & elig & cast_candidate(g, c)
            if hit.any():
                t = np.where(tin > 0, tin, F(0)).astype(F)
                tmin = t[hit].min()
                b = int(np.flatnonzero(hit & (t == tmin))[0])           # smallest t, then the lowest index
                out["body"][q] = b
                out["t"][q] = tmin
                kind = -1
                if not tin[b] < 0:
                    p, r = int(part[b]), F(c[2])
                    kind = p
                    if p == BODY:
                        R = r + g.hx[b]
                        out["normal"][q] = (nx[b] / R, ny[b] / R)
                    elif p >= 2:
                        lx = nx[b] / r
                        ly = ny[b] / r
                        out["normal"][q] = (g.xvx[b] * lx + g.yvx[b] * ly, g.xvy[b] * lx + g.yvy[b] * ly)
                    else:
                        px = ox[b] + tin[b] * dxp[b]                      # the centre at the entry, in the frame
                        py = oy[b] + tin[b] * dyp[b]
                        xface = np.abs(px) - g.hx[b] >= np.abs(py) - g.hy[b]
                        kind = (p, "x" if xface else "y")
                        n, flip = ((g.xvx[b], g.xvy[b]), px < 0) if xface else ((g.yvx[b], g.yvy[b]), py < 0)
                        out["normal"][q] = (-n[0], -n[1]) if flip else n
        if detail is not None:
            detail.append(kind)
    return out
