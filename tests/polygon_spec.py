"""The specification of convex polygon bodies (include/phyx_amd.h POLYGONS), in numpy float32: the definition the device matches byte
for byte (tests/test_polygons_gpu.py) and the host instantiation of the C++ the device kernel calls is held to
(phx_debug_update_manifold_polygons, tests/test_polygons_cpu.py).  tests/polygon_reference.py is its float64 judge.

Every operation is a float32 one, rounded on its own, in the header's order; sqrt and / are correctly rounded;
dot(a, b) = a.x*b.x + a.y*b.y, cross(a, b) = a.x*b.y - a.y*b.x.  A polygon is (count, v): count in 3 .. 8 and v an (8, 2) array of
body-local vertices, counter-clockwise, the unused slots +0.

  poly_valid / normals / frame_box   what phx_world_set_polygons accepts, the stored normals, the frame box it sets
  record / shown                     the stored record {count, v[8], n[8]} and what phx_world_get_polygons returns of it
  poly_poly / disc_polygon / capsule_polygon   the three routines; a box is the 4-gon of its half extents with exact normals
  contacts / update_manifold         UpdateManifolds of one pair: the new points, the reference's MergeCollision once per point, the
                                     two-slot store; pairs without a polygon are capsule_spec's
  masses                             polygon_inverse_masses' formula
  spawn / remove / set_state         the state transforms of the polygon column beside the kinds
  query_points / raycast             the queries with the polygon predicates for the bodies that are polygons
  as_frame_boxes                     the kinds as the four shape queries see them: a polygon is its frame box"""
import numpy as np

from phyx_amd.api import contact_point_dtype, ray_hit_dtype
import capsule_spec as ks
import circle_spec as cs
import query_spec as qs

F = np.float32
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
MAX_VERTICES = 8
MERGE_DISTANCE = F(2.0)
FLT_MAX = cs.FLT_MAX
polygon_dtype = np.dtype([("count", "<i4"), ("v", "<f4", (8, 2))])      # phx_polygon
assert polygon_dtype.itemsize == 68


def polygon(vertices):
    """A phx_polygon of the given vertices (unused slots +0)."""
    p = np.zeros((), dtype=polygon_dtype)
    v = np.asarray(vertices, dtype=F).reshape(-1, 2)
    p["count"] = len(v)
    p["v"][:min(len(v), 8)] = v[:8]
    return p


def regular(n, r, phase=0.0):
    """A regular n-gon of circumradius r, counter-clockwise."""
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return polygon(np.stack([r * np.cos(a), r * np.sin(a)], axis=1))


NONE = polygon(np.zeros((0, 2)))


# ---- validity, normals, the frame box -----------------------------------------------------------------------------------------------------
def normals(count, v):
    """n_k of edge v_k -> v_(k+1): e = v_next - v_k, l = sqrt(dot(e, e)), n = (e.y / l, -e.x / l); an (8, 2) float32 array."""
    v = np.asarray(v, dtype=F).reshape(8, 2)
    n = np.zeros((8, 2), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(count):
            k1 = k + 1 if k + 1 < count else 0
            ex, ey = v[k1, 0] - v[k, 0], v[k1, 1] - v[k, 1]
            l = np.sqrt(ex * ex + ey * ey)
            n[k] = (ey / l, -ex / l)
    return n


def poly_valid(p):
    """What phx_world_set_polygons accepts of one polygon."""
    count = int(p["count"])
    if count < 3 or count > MAX_VERTICES:
        return False
    v = np.asarray(p["v"], dtype=F)
    if not np.isfinite(v[:count]).all():
        return False
    n = normals(count, v)
    with np.errstate(all="ignore"):
        for k in range(count):
            k1 = k + 1 if k + 1 < count else 0
            k2 = k1 + 1 if k1 + 1 < count else 0
            e0x, e0y = v[k1, 0] - v[k, 0], v[k1, 1] - v[k, 1]
            e1x, e1y = v[k2, 0] - v[k1, 0], v[k2, 1] - v[k1, 1]
            if not e0x * e1y - e0y * e1x > 0:
                return False
            if not n[k, 0] * v[k, 0] + n[k, 1] * v[k, 1] > 0:
                return False
    return True


def frame_box(p):
    """geom_size = {max |v_k.x|, max |v_k.y|}."""
    v = np.abs(np.asarray(p["v"], dtype=F)[:int(p["count"])])
    return F(v[:, 0].max()), F(v[:, 1].max())


def shown(p):
    """What phx_world_get_polygons returns of a body that was given p: the count and the vertices, the unused slots +0."""
    out = np.zeros((), dtype=polygon_dtype)
    out["count"] = p["count"]
    out["v"][:int(p["count"])] = p["v"][:int(p["count"])]
    return out


# ---- the state transforms: a list of polygons (NONE where a body is no polygon) beside the kinds ----------------------------------------------
def spawn(polys, count):
    return list(polys) + [NONE] * count


def remove(polys, keep):
    return [p for p, k in zip(polys, keep) if k]


def set_state(n):
    return [NONE] * n


def masses(vertices):
    """{invMass, invInertia} of a polygon on AddBody's scale: float64 shoelace area A and second moment J about the origin,
    mass = 1e-5 * A / 4, inertia = 3 * mass * J / A, both rounded to float32."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    w = np.roll(v, -1, axis=0)
    c = v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1]
    A = 0.5 * c.sum()
    J = (c * ((v * v).sum(1) + (v * w).sum(1) + (w * w).sum(1))).sum() / 12.0
    mass = 1e-5 * A / 4.0
    inertia = 3.0 * mass * J / A
    return F(1.0) / F(mass), F(1.0) / F(inertia)


# ---- the narrowphase ----------------------------------------------------------------------------------------------------------------------
class Body(cs.Body):
    """What the narrowphase reads of a body: the record's fields, the kind and, of a polygon or a box, count, v and n.  A box is the 4-gon
    (-hx,-hy), (hx,-hy), (hx,hy), (-hx,hy) with the exact normals (0,-1), (1,0), (0,1), (-1,0)."""

    def __init__(self, rec, kind, poly=None):
        cs.Body.__init__(self, rec, kind)
        if self.kind == POLYGON:
            self.count = int(poly["count"])
            self.v = np.asarray(poly["v"], dtype=F).reshape(8, 2).copy()
            self.n = normals(self.count, self.v)
        else:
            self.count = 4
            self.v = np.array([(-self.hx, -self.hy), (self.hx, -self.hy), (self.hx, self.hy), (-self.hx, self.hy)], dtype=F)
            self.n = np.array([(0, -1), (1, 0), (0, 1), (-1, 0)], dtype=F)

    def wv(self, k):
        """World vertex (pos + xv*v.x) + yv*v.y."""
        x, y = self.v[k]
        return (self.px + self.xvx * x) + self.yvx * y, (self.py + self.xvy * x) + self.yvy * y

    def wn(self, k):
        """World normal xv*n.x + yv*n.y."""
        x, y = self.n[k]
        return self.xvx * x + self.yvx * y, self.xvy * x + self.yvy * y


def _dot(ax, ay, bx, by):
    return ax * bx + ay * by


def face_sep(a, b, trace=None):
    """(s, i): s_i = min_j dot(NA_i, wB_j - wA_i), the largest s_i, the first on a tie."""
    best, bi, tie = None, 0, False
    for i in range(a.count):
        wx, wy = a.wv(i)
        nx, ny = a.wn(i)
        s = None
        for j in range(b.count):
            bx, by = b.wv(j)
            d = _dot(nx, ny, bx - wx, by - wy)
            if s is None or d < s:
                s = d
        if best is not None and s == best:
            tie = True
        if best is None or s > best:
            best, bi, tie = s, i, False
    if trace is not None:
        trace.append(tie)
    return best, bi


def _clip(p0, p1, d0, d1, trace, name):
    if d0 < 0 and d1 < 0:
        trace.append(name + ":out")
        return None
    if d0 < 0:
        t = d0 / (d0 - d1)
        p0 = (p0[0] + (p1[0] - p0[0]) * t, p0[1] + (p1[1] - p0[1]) * t)
        trace.append(name + ":p0")
    elif d1 < 0:
        t = d1 / (d1 - d0)
        p1 = (p1[0] + (p0[0] - p1[0]) * t, p1[1] + (p0[1] - p1[1]) * t)
        trace.append(name + ":p1")
    return p0, p1


def poly_poly(b1, b2, trace=None):
    """Polygon / polygon and polygon / box: a list of up to two points {p1, p2, n, depth}.  `trace` (a dict) receives which arm was taken:
    ref ("A" or "B", or None where the pair is apart), ref_edge, inc_edge, clips (which end each side plane cut), kept, face_tie (sA or
    sB was reached by two faces), ab_tie (sB == sA), inc_tie (two edges of the incident body equally anti-parallel), touch (an s == 0)."""
    t = {"ref": None, "ref_edge": None, "inc_edge": None, "clips": [], "kept": 0, "face_tie": False, "ab_tie": False, "inc_tie": False, "touch": False}
    if trace is not None:
        trace.update(t)
        t = trace
    with np.errstate(all="ignore"):
        ties = []
        sa, ia = face_sep(b1, b2, ties)
        if sa > 0:
            return []
        sb, ib = face_sep(b2, b1, ties)
        if sb > 0:
            return []
        ref_first = not sb > sa
        R, I, ri = (b1, b2, ia) if ref_first else (b2, b1, ib)
        t.update(ref="A" if ref_first else "B", ref_edge=ri, ab_tie=bool(sa == sb), face_tie=bool(ties[0] if ref_first else ties[1]))
        r0, r1 = R.wv(ri), R.wv(ri + 1 if ri + 1 < R.count else 0)
        nrx, nry = R.wn(ri)
        inc, least = 0, None
        for j in range(I.count):
            nx, ny = I.wn(j)
            d = _dot(nrx, nry, nx, ny)
            if least is not None and d == least:
                t["inc_tie"] = True
            if least is None or d < least:
                least, inc = d, j
                t["inc_tie"] = False
        t["inc_edge"] = inc
        p0, p1 = I.wv(inc), I.wv(inc + 1 if inc + 1 < I.count else 0)
        ex, ey = r1[0] - r0[0], r1[1] - r0[1]
        cut = _clip(p0, p1, _dot(p0[0] - r0[0], p0[1] - r0[1], ex, ey), _dot(p1[0] - r0[0], p1[1] - r0[1], ex, ey), t["clips"], "lo")
        if cut is None:
            return []
        p0, p1 = cut
        cut = _clip(p0, p1, _dot(r1[0] - p0[0], r1[1] - p0[1], ex, ey), _dot(r1[0] - p1[0], r1[1] - p1[1], ex, ey), t["clips"], "hi")
        if cut is None:
            return []
        out = []
        for p in cut:
            s = _dot(nrx, nry, p[0] - r0[0], p[1] - r0[1])
            if not s <= 0:
                continue
            t["touch"] = t["touch"] or bool(s == 0)
            on_ref = (p[0] - nrx * s, p[1] - nry * s)
            if ref_first:
                out.append({"p1": on_ref, "p2": p, "n": (-nrx, -nry), "depth": -s})
            else:
                out.append({"p1": p, "p2": on_ref, "n": (nrx, nry), "depth": -s})
        t["kept"] = len(out)
        return out


def disc_polygon(cx, cy, r, P, disc_first, trace=None):
    """The disc {(cx, cy), r} against polygon (or 4-gon box) P: a candidate or None.  `trace` (a dict) receives region ("inside", "face",
    "vertex_lo", "vertex_hi" or None), edge, tie (two edges share the largest s) and what sat exactly on a boundary."""
    t = {} if trace is None else trace
    t.update(region=None, edge=None, tie=False, t0=False, tee=False, touch=False)
    with np.errstate(all="ignore"):
        gx, gy = cx - P.px, cy - P.py
        px, py = _dot(gx, gy, P.xvx, P.xvy), _dot(gx, gy, P.yvx, P.yvy)
        k, s = 0, None
        for j in range(P.count):
            d = _dot(P.n[j, 0], P.n[j, 1], px - P.v[j, 0], py - P.v[j, 1])
            if s is not None and d == s:
                t["tie"] = True
            if s is None or d > s:
                s, k = d, j
                t["tie"] = False
        t["edge"] = k
        if s > r:
            return None
        vkx, vky = P.v[k]
        nkx, nky = P.n[k]
        Nx, Ny = nkx, nky
        qx, qy = px - nkx * s, py - nky * s
        depth = r - s
        region = "inside"
        if s > 0:
            k1 = k + 1 if k + 1 < P.count else 0
            vnx, vny = P.v[k1]
            ex, ey = vnx - vkx, vny - vky
            tt = _dot(px - vkx, py - vky, ex, ey)
            ee = _dot(ex, ey, ex, ey)
            t["t0"], t["tee"] = bool(tt == 0), bool(tt == ee)
            lo = tt < 0
            hi = (not lo) and tt > ee
            region = "vertex_lo" if lo else ("vertex_hi" if hi else "face")
            if lo or hi:
                qx, qy = (vkx, vky) if lo else (vnx, vny)
                hx, hy = px - qx, py - qy
                l2 = _dot(hx, hy, hx, hy)
                if l2 > r * r:
                    return None
                t["touch"] = bool(l2 == r * r)
                l = np.sqrt(l2)
                Nx, Ny = hx / l, hy / l
                depth = r - l
        t["region"] = region
        wNx, wNy = P.xvx * Nx + P.yvx * Ny, P.xvy * Nx + P.yvy * Ny
        on_poly = ((P.px + P.xvx * qx) + P.yvx * qy, (P.py + P.xvy * qx) + P.yvy * qy)
        on_disc = (cx - wNx * r, cy - wNy * r)
        return ks._cand(on_disc, on_poly, (wNx, wNy), depth, disc_first)


def capsule_polygon(K, P, capsule_first, trace=None):
    """The candidates of capsule K against polygon P as (name, candidate or None): end0, end1, then vertex0 .. in index order, each only
    if unclamped.  `trace` (a dict) receives `clamped`: the vertices that met the capsule nearest an end of its core."""
    e0, e1 = ks.ends(K)
    out = [("end0", disc_polygon(e0[0], e0[1], K.hy, P, capsule_first)), ("end1", disc_polygon(e1[0], e1[1], K.hy, P, capsule_first))]
    clamped = []
    for k in range(P.count):
        x, y = P.wv(k)
        c, unclamped = ks.disc_capsule(x, y, F(0), K, not capsule_first)
        if c is not None and not unclamped:
            clamped.append("vertex%d" % k)
        out.append(("vertex%d" % k, c if unclamped else None))
    if trace is not None:
        trace["clamped"] = clamped
    return out


def contacts(b1, b2, trace=None):
    """The new points of a pair with a polygon, in order: a list of up to two {p1, p2, n, depth}."""
    first = b1.kind == POLYGON
    P, O = (b1, b2) if first else (b2, b1)
    if O.kind == CIRCLE:
        c = disc_polygon(O.px, O.py, O.hx, P, not first, trace)
        return [] if c is None else [c]
    if O.kind == CAPSULE:
        a, b = ks.select(capsule_polygon(O, P, not first, trace), trace)
        return [c for c in (a, b) if c is not None]
    return poly_poly(b1, b2, trace)


def merge(b1, b2, point_count, pts, hits):
    """The reference's MergeCollision once per new point and the two-slot store (as capsule_spec.update_manifold's tail)."""
    work = []
    for k in range(int(point_count)):
        q = pts[k]
        work.append({"d1": (F(q["delta1"]["x"]), F(q["delta1"]["y"])), "d2": (F(q["delta2"]["x"]), F(q["delta2"]["y"])),
                     "n": (F(q["normal"]["x"]), F(q["normal"]["y"])), "merged": 0, "new": 0, "pad": q["pad"].copy(), "si": int(q["solver_index"])})
    sq = lambda ax, ay: ax * ax + ay * ay      # noqa: E731
    for hit in hits:
        with np.errstate(all="ignore"):
            p1, p2, n = hit["p1"], hit["p2"], hit["n"]
            d1 = (p1[0] - b1.px, p1[1] - b1.py)
            d2 = (p2[0] - b2.px, p2[1] - b2.py)
            closest, best = -1, FLT_MAX
            for i, q in enumerate(work):
                s1 = sq(q["d1"][0] - d1[0], q["d1"][1] - d1[1])
                s2 = sq(q["d2"][0] - d2[0], q["d2"][1] - d2[1])
                if s1 > MERGE_DISTANCE * MERGE_DISTANCE and s2 > MERGE_DISTANCE * MERGE_DISTANCE:
                    continue
                depth = sq(d1[0] - q["d1"][0], d1[1] - q["d1"][1]) + sq(d2[0] - q["d2"][0], d2[1] - q["d2"][1])
                if depth < best:
                    best, closest = depth, i
        if closest >= 0:
            work[closest].update(d1=d1, d2=d2, n=n, merged=1, new=0)
        else:
            work.append({"d1": d1, "d2": d2, "n": n, "merged": 1, "new": 1, "pad": np.zeros(2, dtype=np.uint8), "si": -1})
    out = np.array(pts[:2], dtype=contact_point_dtype).copy()
    count = 0
    for q in work:
        if not q["merged"]:
            continue
        assert count < 2
        o = out[count]
        o["delta1"]["x"], o["delta1"]["y"] = q["d1"]
        o["delta2"]["x"], o["delta2"]["y"] = q["d2"]
        o["normal"]["x"], o["normal"]["y"] = q["n"]
        o["is_merged"], o["is_newly_created"], o["pad"], o["solver_index"] = q["merged"], q["new"], q["pad"], q["si"]
        count += 1
    return count, out


def update_manifold(rec1, kind1, poly1, rec2, kind2, poly2, point_count, pts):
    """UpdateManifolds of one pair; poly1, poly2: the bodies' polygons (None or NONE where a body is none)."""
    if kind1 != POLYGON and kind2 != POLYGON:
        return ks.update_manifold(rec1, kind1, rec2, kind2, point_count, pts)
    b1, b2 = Body(rec1, kind1, poly1), Body(rec2, kind2, poly2)
    return merge(b1, b2, point_count, pts, contacts(b1, b2))


# ---- the queries --------------------------------------------------------------------------------------------------------------------------
def as_frame_boxes(kinds):
    """The kinds as oriented-box overlap, box casts, circle overlap and circle casts see them: a polygon is its frame box."""
    k = np.asarray(kinds, dtype=np.int32).copy()
    k[k == POLYGON] = BOX
    return k


def _frame_point(g, b, x, y):
    dx, dy = x - g.px[b], y - g.py[b]
    return dx * g.xvx[b] + dy * g.xvy[b], dx * g.yvx[b] + dy * g.yvy[b]


def point_in_polygon(g, b, poly, x, y):
    """The AABB conjunct AND every dot(n_k, p' - v_k) <= 0, for body b."""
    x, y = F(x), F(y)
    with np.errstate(all="ignore"):
        if not (g.lox[b] <= x and g.hix[b] >= x and g.loy[b] <= y and g.hiy[b] >= y):
            return False
        u, v = _frame_point(g, b, x, y)
        count, vs = int(poly["count"]), np.asarray(poly["v"], dtype=F)
        n = normals(count, vs)
        return all(n[k, 0] * (u - vs[k, 0]) + n[k, 1] * (v - vs[k, 1]) <= 0 for k in range(count))


def ray_polygon(g, b, poly, r):
    """(pass, tin, entering edge or -1) of ray r = (ox, oy, dx, dy, max_t) against body b's polygon, in the body's frame."""
    ox, oy, dx, dy, max_t = (F(v) for v in r)
    with np.errstate(all="ignore"):
        oxp, oyp = _frame_point(g, b, ox, oy)
        dxp = dx * g.xvx[b] + dy * g.xvy[b]
        dyp = dx * g.yvx[b] + dy * g.yvy[b]
        count, vs = int(poly["count"]), np.asarray(poly["v"], dtype=F)
        n = normals(count, vs)
        tin, tout, edge, miss = F(-np.inf), F(np.inf), -1, False
        for k in range(count):
            den = n[k, 0] * dxp + n[k, 1] * dyp
            num = n[k, 0] * (vs[k, 0] - oxp) + n[k, 1] * (vs[k, 1] - oyp)
            if den < 0:
                t = num / den
                if t > tin:
                    tin, edge = t, k
            elif den > 0:
                t = num / den
                if t < tout:
                    tout = t
            elif num < 0:
                miss = True
        return bool((not miss) and tin <= tout and tout >= 0 and tin <= max_t), tin, edge


def query_points(bodies, kinds, polys, points, skip_static=False):
    g = qs.Geometry(bodies)
    kd = np.asarray(kinds, dtype=np.int32)
    pts = np.asarray(points, dtype=F).reshape(-1, 2)
    out = np.full(len(pts), -1, dtype=np.int32)
    elig = g.eligible(skip_static)
    for q, p in enumerate(pts):
        if not qs.point_ok(p) or not g.n:
            continue
        inside = np.where(kd == CAPSULE, ks.point_in_capsule(g, p[0], p[1]),
                          np.where(kd == CIRCLE, cs.point_in_circle(g, p[0], p[1]), qs.point_in_box(g, p[0], p[1])))
        for b in np.flatnonzero(kd == POLYGON):
            inside[b] = point_in_polygon(g, b, polys[b], p[0], p[1])
        hit = np.flatnonzero(elig & inside)
        if len(hit):
            out[q] = hit[0]
    return out


def raycast(bodies, kinds, polys, rays, skip_static=False):
    """capsule_spec.raycast with the polygon rule for the bodies that are polygons."""
    g = qs.Geometry(bodies)
    kd = np.asarray(kinds, dtype=np.int32)
    rs = np.asarray(rays, dtype=F).reshape(-1, 5)
    out = ks.raycast(bodies, as_frame_boxes(kd), rays, skip_static)
    if not (kd == POLYGON).any():
        return out
    elig = g.eligible(skip_static)
    for q, r in enumerate(rs):
        if not (qs.ray_ok(r) and g.n):
            continue
        ox, oy, dx, dy, max_t = (F(v) for v in r)
        cand = qs.ray_candidate(g, r)
        best = None                                                            # (t, body, tin, edge)
        for b in np.flatnonzero((kd == POLYGON) & elig & cand):
            ok, tin, edge = ray_polygon(g, b, polys[b], r)
            if ok:
                t = tin if tin > 0 else F(0)
                if best is None or t < best[0]:
                    best = (t, int(b), tin, edge)
        rest = _raycast_without(bodies, kd, r, skip_static)
        take_poly = best is not None and (rest["body"] < 0 or best[0] < rest["t"] or (best[0] == rest["t"] and best[1] < rest["body"]))
        if not take_poly:
            out[q] = rest
            continue
        t, b, tin, edge = best
        out["body"][q], out["t"][q], out["normal"][q] = b, t, (0, 0)
        if not tin < 0 and edge >= 0:
            n = normals(int(polys[b]["count"]), polys[b]["v"])[edge]
            with np.errstate(all="ignore"):
                out["normal"][q] = (g.xvx[b] * n[0] + g.yvx[b] * n[1], g.xvy[b] * n[0] + g.yvy[b] * n[1])
        with np.errstate(all="ignore"):
            out["point"][q] = (ox + t * dx, oy + t * dy)
    return out


def _raycast_without(bodies, kd, r, skip_static):
    """The ray against the bodies that are no polygons, indices kept: the polygons are made ineligible by an empty AABB (min > max fails
    the candidate test, query_spec.ray_candidate)."""
    b = np.array(bodies, copy=True)
    poly = kd == POLYGON
    b["aabb_min"]["x"][poly] = F(1)
    b["aabb_max"]["x"][poly] = F(-1)
    return ks.raycast(b, as_frame_boxes(kd), np.asarray(r, dtype=F).reshape(1, 5), skip_static)[0]
