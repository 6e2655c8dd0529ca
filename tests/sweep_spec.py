"""Continuous bodies stated in numpy (include/phyx_amd.h CONTINUOUS BODIES): the float32 definition the device equals byte for byte.

A continuous body has a core radius rc > 0.  After a step's IntegratePosition its core disc {s, rc} is cast along d = e - s (s: the
position before the integrator ran, e: after it) against every target, and the body is put back a skin (rc / 64) short of the earliest
touch t:   t' = max(t - skin / approach, 0),   pos = (s.x + d.x*t', s.y + d.y*t'),   the AABB by UpdateGeom on the new position and
the frame the integrator left.  The header says why the skin is there; it also bounds what counts as approaching (sweep).
Every formula is one float32 operation at a time.  The casts against boxes, circle bodies and capsules are the circle casts of
tests/round_query_spec.py and tests/capsule_spec.py with max_t = 1, their AABB conjunct included, taken from there and not restated;
the cast against a polygon's true outline is stated here (cast_polygon).

  column state     spawn / remove / set_state: what the per-body core radii do between steps
  inradius         min(hx, hy) of a box, r of a circle, hy of a capsule, min_k dot(n_k, v_k) of a polygon
  targets          who a swept body is cast against
  cast_target      one target: (hit, t, normal, label)
  sweep            the pass: (bodies after it, hits)"""
import numpy as np

from phyx_amd.api import sweep_hit_dtype
import capsule_spec as ks
import filter_spec
import polygon_spec as ps
import query_spec as qs
import round_query_spec as rq

F = np.float32
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
SENSOR = 1


def skin(rc):
    """rc * 2^-6 (include/phyx_amd.h CONTINUOUS BODIES, the skin): a hit counts only if the step approaches the target by more than this,
    and a clamped body is put back this far short of the first touch."""
    return F(F(rc) * F(0.015625))


# ---- the column between steps ---------------------------------------------------------------------------------------------------------
def spawn(rc, count):
    return np.concatenate([np.asarray(rc, dtype=F), np.zeros(count, dtype=F)])


def remove(rc, keep):
    return np.asarray(rc, dtype=F)[np.asarray(keep, dtype=bool)]


def set_state(n):
    return np.zeros(n, dtype=F)


def inradius(kind, hx, hy, poly=None):
    if kind == CIRCLE:
        return F(hx)
    if kind == CAPSULE:
        return F(hy)
    if kind == POLYGON:
        count = int(poly["count"])
        v = np.asarray(poly["v"], dtype=F).reshape(8, 2)
        n = ps.normals(count, v)
        return min(F(F(n[k, 0] * v[k, 0]) + F(n[k, 1] * v[k, 1])) for k in range(count))
    return min(F(hx), F(hy))


def valid(kind, hx, hy, rc, poly=None):
    """What phx_world_set_continuous accepts of one body: rc finite, >= 0 and, where above 0, strictly below the inradius."""
    rc = F(rc)
    if not (np.isfinite(rc) and rc >= 0):
        return False
    return bool(rc == 0 or rc < inradius(kind, hx, hy, poly))


# ---- the targets ----------------------------------------------------------------------------------------------------------------------
def targets(bodies, i, flags=None, filters=None, exclusions=None, only=None):
    """The bodies body i is cast against: both inverse masses read 0 (a sleeper's do), no sensor on either side, the collision filters
    pass, the pair is not excluded.  `exclusions`: an (n, 2) list of body pairs.  `only`: a mask of the bodies the caller asks about
    (the filter rule is evaluated for those alone)."""
    b = np.asarray(bodies)
    n = len(b)
    t = (b["inv_mass"] == 0) & (b["inv_inertia"] == 0)
    if flags is not None:
        f = np.asarray(flags, dtype=np.uint32)
        t &= (f & SENSOR) == 0
        if f[i] & SENSOR:
            t[:] = False
    if filters is not None:
        for j in np.flatnonzero(t if only is None else t & only):
            t[j] = filter_spec.should_collide(filters[i], filters[j])
    if exclusions is not None:
        for a, c in np.asarray(exclusions, dtype=np.int64).reshape(-1, 2):
            if a == i:
                t[c] = False
            if c == i:
                t[a] = False
    t[i] = False
    return t


# ---- the cast against a polygon's outline ---------------------------------------------------------------------------------------------
def cast_polygon(rec, poly, sx, sy, rc, dx, dy):
    """The disc {s, rc} along d, t in [0, 1], against the polygon of record `rec`, in the polygon's frame: (hit, t, (nx, ny) world, label).
    label: "overlap" (the start overlaps: no hit), ("face", k), ("vertex", k) or None."""
    px, py = F(rec["pos"]["x"]), F(rec["pos"]["y"])
    xvx, xvy, yvx, yvy = F(rec["xv"]["x"]), F(rec["xv"]["y"]), F(rec["yv"]["x"]), F(rec["yv"]["y"])
    count = int(poly["count"])
    v = np.asarray(poly["v"], dtype=F).reshape(8, 2)
    n = ps.normals(count, v)
    sx, sy, rc, dx, dy = F(sx), F(sy), F(rc), F(dx), F(dy)
    with np.errstate(all="ignore"):
        rx, ry = sx - px, sy - py
        ox, oy = rx * xvx + ry * xvy, rx * yvx + ry * yvy
        dxp, dyp = dx * xvx + dy * xvy, dx * yvx + dy * yvy
        # the start: the explicit distance test
        k, s = 0, n[0, 0] * (ox - v[0, 0]) + n[0, 1] * (oy - v[0, 1])
        for j in range(1, count):
            c = n[j, 0] * (ox - v[j, 0]) + n[j, 1] * (oy - v[j, 1])
            if c > s:
                s, k = c, j
        if s <= 0:
            return False, F(0), (F(0), F(0)), "overlap"
        k1 = k + 1 if k + 1 < count else 0
        ex, ey = v[k1, 0] - v[k, 0], v[k1, 1] - v[k, 1]
        u = (ox - v[k, 0]) * ex + (oy - v[k, 1]) * ey
        lo = u < 0
        hi = (not lo) and u > ex * ex + ey * ey
        if lo or hi:
            q = v[k] if lo else v[k1]
            hx, hy = ox - q[0], oy - q[1]
            if hx * hx + hy * hy < rc * rc:
                return False, F(0), (F(0), F(0)), "overlap"
        elif s < rc:
            return False, F(0), (F(0), F(0)), "overlap"
        hit, best, bn, label = False, F(0), (F(0), F(0)), None
        for k in range(count):                                              # the faces, pushed out by rc and kept to their own extent
            k1 = k + 1 if k + 1 < count else 0
            nx, ny, vx, vy = n[k, 0], n[k, 1], v[k, 0], v[k, 1]
            den = nx * dxp + ny * dyp
            if not den < 0:
                continue
            t = ((nx * (vx - ox) + ny * (vy - oy)) + rc) / den
            if not (t >= 0 and t <= 1):
                continue
            ex, ey = v[k1, 0] - vx, v[k1, 1] - vy
            qx, qy = ox + dxp * t, oy + dyp * t
            u = (qx - vx) * ex + (qy - vy) * ey
            if not (u >= 0 and u <= ex * ex + ey * ey):
                continue
            if not hit or t < best:
                hit, best, bn, label = True, t, (nx, ny), ("face", k)
        for k in range(count):                                              # the vertices: the ray/disc rule with radius rc
            ok, tin, nx, ny = rq.ray_disc(ox - v[k, 0], oy - v[k, 1], dxp, dyp, F(1), rc)
            if not ok or tin < 0:
                continue
            if not hit or tin < best:
                hit, best, bn, label = True, F(tin), (F(nx / rc), F(ny / rc)), ("vertex", k)
        if not hit:
            return False, F(0), (F(0), F(0)), None
        return True, F(best), (F(xvx * bn[0] + yvx * bn[1]), F(xvy * bn[0] + yvy * bn[1])), label


# ---- one target -----------------------------------------------------------------------------------------------------------------------
def cast_target(rec, kind, poly, sx, sy, rc, dx, dy):
    """The core disc against one target by its kind: (hit, t, normal, label).  Boxes, circle bodies and capsules: the header's circle
    cast {s, rc, d, 1} against this one body (its AABB conjunct included); a start inside the widened shape (tin < 0: the core overlaps the
    target at t = 0) is no hit."""
    if int(kind) == POLYGON:
        g = qs.Geometry(np.asarray(rec).reshape(1))
        c = np.array([sx, sy, rc, dx, dy, 1], dtype=F)
        if not rq.cast_candidate(g, c)[0]:
            return False, F(0), (F(0), F(0)), None
        return cast_polygon(rec, poly, sx, sy, rc, dx, dy)
    one = np.asarray(rec).reshape(1)
    c = np.array([[sx, sy, rc, dx, dy, 1]], dtype=F)
    if not rq.cast_candidate(qs.Geometry(one), c[0])[0]:
        return False, F(0), (F(0), F(0)), None
    detail, tins = [], []
    h = _cast_one(one, int(kind), c[0], detail, tins)
    if h is None:
        return False, F(0), (F(0), F(0)), None
    if tins[0] < 0:
        return False, F(0), (F(0), F(0)), "overlap"
    return True, F(h["t"]), (F(h["normal"][0]), F(h["normal"][1])), detail[0]


def _cast_one(one, kind, c, detail, tins):
    """capsule_spec.cast_circles on the one body, and the raw tin of its winner (the queries clamp t to 0 and drop the normal there)."""
    g = qs.Geometry(one)
    kd = np.array([kind], dtype=np.int32)
    h = ks.cast_circles(one, kd, [c], detail=detail)[0]
    if h["body"] < 0:
        return None
    cx, cy, r, dx, dy, max_t = (F(v) for v in c)
    if kind == CAPSULE:
        with np.errstate(all="ignore"):
            tins.append(ks.ray_capsule(g, cx - g.px, cy - g.py, dx, dy, max_t, r + g.hy)[1][0])
    else:
        tins.append(rq.cast_body(g, kd == CIRCLE, c)[1][0])
    return h


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------
def update_geom(rec):
    """UpdateGeom's AABB (ref: Geom.h:79-85) of a record whose pos changed: pos -/+ (|xv|*h.x + |yv|*h.y), and the geom copies of pos."""
    px, py = F(rec["pos"]["x"]), F(rec["pos"]["y"])
    hx, hy = F(rec["geom_size"]["x"]), F(rec["geom_size"]["y"])
    ex = np.abs(F(rec["xv"]["x"])) * hx + np.abs(F(rec["yv"]["x"])) * hy
    ey = np.abs(F(rec["xv"]["y"])) * hx + np.abs(F(rec["yv"]["y"])) * hy
    rec["geom_pos"] = (px, py)
    rec["aabb_min"] = (px - ex, py - ey)
    rec["aabb_max"] = (px + ex, py + ey)


def sweep(bodies, start, rc, kinds=None, polys=None, flags=None, filters=None, exclusions=None, detail=None):
    """The pass on `bodies` (the records behind IntegratePosition) with `start` (n, 2), the positions in front of it, and rc (n,) the
    core radii: (records after the pass, hits as sweep_hit_dtype ascending by body).  A target's hit counts only if the step approaches
    it by more than the skin; the smallest t wins, ties to the lowest index; the body is put back a skin short of that touch,
    t' = max(t - skin / approach, 0) with approach = -dot(normal, d), and the hit records t'.  `detail` (a dict) receives per swept
    body the label of every target it considered and, under ("touch", body), the winner's t before the skin was taken off."""
    out = np.array(bodies, copy=True)
    n = len(out)
    kd = np.zeros(n, dtype=np.int32) if kinds is None else np.asarray(kinds, dtype=np.int32)
    rc = np.asarray(rc, dtype=F)
    start = np.asarray(start, dtype=F).reshape(n, 2)
    g = qs.Geometry(bodies)
    hits = []
    for i in range(n):
        if not rc[i] > 0:
            continue
        if bodies[i]["inv_mass"] == 0 and bodies[i]["inv_inertia"] == 0:
            continue
        sx, sy = start[i]
        dx, dy = F(bodies[i]["pos"]["x"]) - sx, F(bodies[i]["pos"]["y"]) - sy
        if dx == 0 and dy == 0:
            continue
        best = None
        labels = {}
        # (the AABB conjunct of every cast below, for all bodies at once: a target that fails it is no hit, whatever its kind)
        near = rq.cast_candidate(g, np.array([sx, sy, rc[i], dx, dy, 1], dtype=F))
        for j in np.flatnonzero(near & targets(bodies, i, flags, filters, exclusions, only=near)):
            hit, t, nrm, label = cast_target(bodies[j], kd[j], None if polys is None else polys[j], sx, sy, rc[i], dx, dy)
            labels[int(j)] = label
            if not hit:
                continue
            with np.errstate(all="ignore"):
                if not F(nrm[0] * dx) + F(nrm[1] * dy) < -skin(rc[i]):
                    labels[int(j)] = ("away", label)
                    continue
            if best is None or t < best[0]:                                 # (j ascends: the lowest index stays on a tie)
                best = (t, int(j), nrm)
        if detail is not None:
            detail[i] = labels
        if best is None:
            continue
        t, j, nrm = best
        if detail is not None:
            detail[("touch", i)] = t
        with np.errstate(all="ignore"):
            approach = -(F(nrm[0] * dx) + F(nrm[1] * dy))
            back = F(t - F(skin(rc[i]) / approach))
        t = back if back > 0 else F(0)
        out[i]["pos"] = (F(sx + F(dx * t)), F(sy + F(dy * t)))
        update_geom(out[i])
        h = np.zeros((), dtype=sweep_hit_dtype)
        h["body"], h["target"], h["t"], h["normal"] = i, j, t, nrm
        hits.append(h)
    return out, np.array(hits, dtype=sweep_hit_dtype).reshape(-1)
