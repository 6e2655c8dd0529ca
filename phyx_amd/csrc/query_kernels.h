// query_kernels.h — the device side of the World's queries (include/phyx_amd.h, QUERIES): AABB overlap, point in box or disc, the closest
// ray hit, oriented-box overlap and the closest box-cast hit, circle overlap and the closest circle-cast hit, the nearest body of a point over the resident arrays
// (body_view.h).  The predicates below are the header's formulas one for one, each operation rounded on its own (the library is
// compiled with -ffp-contract=off); tests/query_spec.py, tests/shape_query_spec.py, tests/round_query_spec.py, tests/capsule_spec.py and
// tests/near_spec.py state them again in numpy.
//
// Two paths give byte-identical results:
//   scan   bodies in lanes, a tile of Q_TILE queries in LDS, one coalesced pass over the resident arrays per tile; points and rays
//          and casts reduce with atomicMin (the body index; (bits(t) << 32) | body), AABB, box and circle queries count per (query,
//          workgroup), scan, fill;
//   index  a tree of 64-wide nodes over the bodies in Morton order (leaves: 64 consecutive sorted bodies), one wave per query: the
//          64 lanes test one node's 64 children and __ballot picks the ones to descend into; the stack lives in LDS.
// Pruning is exact: a node's bounds are the exact min / max of what it holds, and every test is monotonic in the box it is made
// against (Queries), so a body that passes its own test passes every ancestor's.
#pragma once

#include "body_view.h"
#include "sleep.h"

#include <climits>

namespace phx {

constexpr int Q_TILE = 64;              // queries per scan-path tile (LDS)
constexpr int Q_FANOUT = 64;            // children per tree node: one wave's lanes
constexpr int Q_MAX_LEVELS = 6;         // 64^6 > 2^31 bodies
constexpr int Q_SORT_MAX = 4096;        // AABB segments up to this long are sorted in LDS by one workgroup (16 KiB)
constexpr int Q_SKIP_STATIC = 1;        // PHX_QUERY_SKIP_STATIC

struct QRay { float ox, oy, dx, dy, max_t; };
struct QBox { float px, py, xx, xy, yx, yy, hx, hy; };      // a query box {pos, xv, yv, h}
struct QCast { QBox b; float dx, dy, max_t; };
struct QDisc { float cx, cy, r; };                          // a query circle {c, r}
struct QDiscCast { QDisc c; float dx, dy, max_t; };
// the shape a query brings: none (an AABB, a ray), an oriented box, a circle
enum { QSHAPE_NONE = 0, QSHAPE_BOX = 1, QSHAPE_DISC = 2 };

// the tree: level 0 is the sorted bodies (perm), level L >= 1 holds cnt[L] nodes at nodes[off[L] ..]; node i of level L bounds
// children 64i .. 64i + 63 of level L - 1; the root is the one node of level `levels`
struct QTree {
    const float4* nodes;
    const unsigned* perm;
    int n, levels;
    int off[Q_MAX_LEVELS + 1], cnt[Q_MAX_LEVELS + 1];
};

// ---- the predicates (include/phyx_amd.h) ----------------------------------------------------------------------------------------
// (`sleep`: the sleep column, null while sleeping is off — a sleeper's inverse masses are zeroed, but it is a body at rest, not ground:
//  picking a box out of a resting pile is the first thing a user does)
__device__ __forceinline__ bool q_static(float4 m, const SleepCell* __restrict__ sleep, int i) { return m.x == 0.f && m.y == 0.f && !(sleep && sleep[i].asleep); }

__device__ __forceinline__ bool q_overlap(float4 a, float4 q) { return a.x <= q.z && a.z >= q.x && a.y <= q.w && a.w >= q.y; }

__device__ __forceinline__ bool q_point_in_box(float4 a, float4 m, float4 f, float2 h, float px, float py)
{
    if (!(a.x <= px && a.z >= px && a.y <= py && a.w >= py)) return false;
    const float dx = px - m.z, dy = py - m.w;
    const float u = dx * f.x + dy * f.y, v = dx * f.z + dy * f.w;
    return fabsf(u) <= h.x && fabsf(v) <= h.y;
}

// circles (include/phyx_amd.h SHAPES, QUERIES): `kinds` is the shape column, null while no body is a circle.  A circle's radius is its
// size.x; the AABB conjunct and the candidate test are the box's.  Oriented boxes and box casts see a circle as its frame square; query
// circles and circle casts (the round predicates below) see the disc.
__device__ __forceinline__ bool q_circle(const uint32_t* __restrict__ kinds, int i) { return kinds && kinds[i] != (uint32_t)PHX_SHAPE_BOX; }
// Capsules: every kernel that reads the kinds has a second instantiation, CAPS, which a world launches once some call has named a capsule
// (WorldBodies::capsules; query.hip q_caps).  Without it a kind is 0 or 1, q_circle's answer, and no capsule predicate is compiled in: a
// world of boxes and circles runs the code it always ran.  A capsule's core segment runs along the frame's x from -a to a, a = h.x - h.y,
// its radius is h.y.  Oriented boxes and box casts see a capsule as its frame box {h.x, h.y}, as they see a circle as its frame square.
template <int CAPS>
__device__ __forceinline__ unsigned q_kind(const uint32_t* __restrict__ kinds, int i)
{
    if (CAPS) return kinds ? kinds[i] : (unsigned)PHX_SHAPE_BOX;
    return q_circle(kinds, i) ? 1u : 0u;
}
// Polygons (include/phyx_amd.h POLYGONS): a third instantiation, CAPS == 2, which a world launches once some call has named a polygon
// (WorldBodies::polys).  It holds the capsule predicates too.  Points and rays see the polygon's true outline; query circles, circle casts,
// oriented boxes and box casts see its frame box: wherever a rule says "a kind that is not a box" a polygon takes the box's arm.
template <int CAPS>
__device__ __forceinline__ const PolyRec* q_poly(const WorldBodies& w, int i) { return CAPS == 2 ? w.polys + i : nullptr; }

__device__ __forceinline__ bool q_point_in_polygon(float4 a, float4 m, float4 f, const PolyRec* __restrict__ poly, float px, float py)
{
    if (!(a.x <= px && a.z >= px && a.y <= py && a.w >= py)) return false;
    const float dx = px - m.z, dy = py - m.w;
    const float u = dx * f.x + dy * f.y, v = dx * f.z + dy * f.w;
    const int n = poly->count;
    bool in = true;
    for (int k = 0; k < n; ++k) in = in && poly->n[2 * k] * (u - poly->v[2 * k]) + poly->n[2 * k + 1] * (v - poly->v[2 * k + 1]) <= 0.f;
    return in;
}

// the ray against the polygon's half planes in the body's frame (after the candidate test); `edge`: the entering edge, -1 if none entered
__device__ __forceinline__ bool q_ray_polygon(const QRay& r, float4 m, float4 f, const PolyRec* __restrict__ poly, float& tin, int& edge)
{
    const float rx = r.ox - m.z, ry = r.oy - m.w;
    const float oxp = rx * f.x + ry * f.y, oyp = rx * f.z + ry * f.w;
    const float dxp = r.dx * f.x + r.dy * f.y, dyp = r.dx * f.z + r.dy * f.w;
    const int n = poly->count;
    float tout = INFINITY;
    bool miss = false;
    tin = -INFINITY; edge = -1;
    for (int k = 0; k < n; ++k) {
        const float nx = poly->n[2 * k], ny = poly->n[2 * k + 1];
        const float den = nx * dxp + ny * dyp, num = nx * (poly->v[2 * k] - oxp) + ny * (poly->v[2 * k + 1] - oyp);
        if (den < 0.f) { const float t = num / den; if (t > tin) { tin = t; edge = k; } }
        else if (den > 0.f) { const float t = num / den; if (t < tout) tout = t; }
        else if (num < 0.f) miss = true;
    }
    return !miss && tin <= tout && tout >= 0.f && tin <= r.max_t;
}

__device__ __forceinline__ float q_clamp(float u, float a) { return u < -a ? -a : (u > a ? a : u); }

__device__ __forceinline__ bool q_point_in_capsule(float4 a, float4 m, float4 f, float2 h, float px, float py)
{
    if (!(a.x <= px && a.z >= px && a.y <= py && a.w >= py)) return false;
    const float dx = px - m.z, dy = py - m.w;
    const float u = dx * f.x + dy * f.y, v = dx * f.z + dy * f.w;
    const float ha = h.x - h.y, gx = u - q_clamp(u, ha);
    return gx * gx + v * v <= h.y * h.y;
}

__device__ __forceinline__ bool q_point_in_circle(float4 a, float4 m, float r, float px, float py)
{
    if (!(a.x <= px && a.z >= px && a.y <= py && a.w >= py)) return false;
    const float dx = px - m.z, dy = py - m.w;
    return dx * dx + dy * dy <= r * r;
}

template <int CAPS>
__device__ __forceinline__ bool q_point_in_body(unsigned kind, float4 a, float4 m, float4 f, float2 h, float px, float py, const PolyRec* poly)
{
    if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) return q_point_in_polygon(a, m, f, poly, px, py);
    if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) return q_point_in_capsule(a, m, f, h, px, py);
    return kind != 0u ? q_point_in_circle(a, m, h.x, px, py) : q_point_in_box(a, m, f, h, px, py);
}

// one axis's slab: false when it is empty
__device__ __forceinline__ bool q_slab(float o, float d, float lo, float hi, float& t0, float& t1)
{
    if (d == 0.f) { t0 = -INFINITY; t1 = INFINITY; return lo <= o && o <= hi; }
    const float a = (lo - o) / d, b = (hi - o) / d;
    t0 = a <= b ? a : b; t1 = a <= b ? b : a;
    return true;
}

// the two-axis test over [0, max_t]; tin and which axis entered (x on a tie)
__device__ __forceinline__ bool q_ray_test(float ox, float oy, float dx, float dy, float lox, float loy, float hix, float hiy, float max_t,
                                           float& tin, bool& xenter)
{
    float t0x, t1x, t0y, t1y;
    const bool sx = q_slab(ox, dx, lox, hix, t0x, t1x), sy = q_slab(oy, dy, loy, hiy, t0y, t1y);
    if (!sx || !sy) return false;
    xenter = t0x >= t0y;
    tin = xenter ? t0x : t0y;
    const float tout = t1x <= t1y ? t1x : t1y;
    return tin <= tout && tout >= 0.f && tin <= max_t;
}

// candidate test against an AABB (a body's or a node's bounds)
__device__ __forceinline__ bool q_ray_aabb(const QRay& r, float4 a)
{
    if (!(a.x <= a.z && a.y <= a.w)) return false;
    float tin; bool xe;
    return q_ray_test(r.ox, r.oy, r.dx, r.dy, a.x, a.y, a.z, a.w, r.max_t, tin, xe);
}

struct QRayBox { float tin, dxp, dyp; bool xenter; };

// the test in the body's frame (after the candidate test)
__device__ __forceinline__ bool q_ray_box(const QRay& r, float4 m, float4 f, float2 h, QRayBox& out)
{
    const float rx = r.ox - m.z, ry = r.oy - m.w;
    const float oxp = rx * f.x + ry * f.y, oyp = rx * f.z + ry * f.w;
    out.dxp = r.dx * f.x + r.dy * f.y;
    out.dyp = r.dx * f.z + r.dy * f.w;
    return q_ray_test(oxp, oyp, out.dxp, out.dyp, -h.x, -h.y, h.x, h.y, r.max_t, out.tin, out.xenter);
}

// the ray against the disc (after the candidate test), by the closest approach: tc is where the line passes the centre closest, e the
// offset there, s half the chord in units of t, under the box rule; nx, ny = the entry point from the centre (the normal is n / r).
// Nothing of the size of the origin's distance is squared: a small disc seen from far away keeps its chord.
// (q_ray_disc: the rule with the origin already taken relative to the centre: (rx, ry); a circle cast's corner discs use it in the
// body's frame)
__device__ __forceinline__ bool q_ray_disc(float rx, float ry, float dx, float dy, float max_t, float rad, float& tin, float& nx, float& ny)
{
    const float a = dx * dx + dy * dy, b = rx * dx + ry * dy;
    const float tc = -b / a;
    const float ex = rx + tc * dx, ey = ry + tc * dy;
    const float h2 = rad * rad - (ex * ex + ey * ey);
    tin = 0.f; nx = 0.f; ny = 0.f;
    if (!(h2 >= 0.f)) return false;
    const float s = sqrtf(h2 / a);
    tin = tc - s;
    const float tout = tc + s;
    nx = ex - s * dx; ny = ey - s * dy;
    return tin <= tout && tout >= 0.f && tin <= max_t;
}

__device__ __forceinline__ bool q_ray_circle(const QRay& r, float4 m, float rad, float& tin, float& nx, float& ny)
{
    return q_ray_disc(r.ox - m.z, r.oy - m.w, r.dx, r.dy, r.max_t, rad, tin, nx, ny);
}

// part: 0 the wide box, 1 the tall box, 2 .. 5 the corner discs (-,-) (+,-) (-,+) (+,+), Q_PART_BODY a circle body's own disc;
// of a capsule body: Q_PART_SIDE the box between its ends, Q_PART_END an end disc.
// ox, oy, dxp, dyp: o' and d', the cast in a box's frame (q_ray_box);  nx, ny: a disc part's entry point from its centre (q_ray_disc)
constexpr int Q_PART_BODY = 6, Q_PART_SIDE = 7, Q_PART_END = 8;
struct QCastDisc { float tin; int part; float ox, oy, dxp, dyp, nx, ny; };

// the ray (origin relative to the body: rx, ry) against a capsule of radius R about the core segment of half length ha: the union of
// three convex parts in the frame, each met by its own rule: the box lo = (-ha, -R), hi = (ha, R), then the discs of radius R at (-ha, 0)
// and (ha, 0); the earliest entry wins, the first part in order on a tie.  A ray has R = h.y, a circle cast R = r + h.y.
__device__ __forceinline__ bool q_ray_capsule(float rx, float ry, float dx, float dy, float max_t, float4 f, float ha, float R, QCastDisc& out)
{
    const float ox = rx * f.x + ry * f.y, oy = rx * f.z + ry * f.w;
    out.ox = ox; out.oy = oy;
    out.dxp = dx * f.x + dy * f.y;
    out.dyp = dx * f.z + dy * f.w;
    out.nx = 0.f; out.ny = 0.f; out.part = Q_PART_SIDE;
    float tin = 0.f;
    bool xe = false;
    bool hit = q_ray_test(ox, oy, out.dxp, out.dyp, -ha, -R, ha, R, max_t, tin, xe);
    out.tin = hit ? tin : 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float kx = k ? ha : -ha;
        float nx, ny;
        const bool pass = q_ray_disc(ox - kx, oy, out.dxp, out.dyp, max_t, R, tin, nx, ny);
        const bool better = pass && (!hit || tin < out.tin);
        out.tin = better ? tin : out.tin; out.part = better ? Q_PART_END : out.part;
        out.nx = better ? nx : out.nx; out.ny = better ? ny : out.ny;
        hit = hit || pass;
    }
    return hit;
}

// a capsule hit's normal (tin >= 0): the side's is yv, negated where the entry point lies below the axis (the box part's x faces are
// interior: the face is chosen by where the point is); an end's is the frame normal n / R turned into the world
__device__ __forceinline__ float2 q_capsule_normal(const QCastDisc& cd, float4 f, float R)
{
    if (cd.part == Q_PART_SIDE) {
        const bool flip = cd.oy + cd.tin * cd.dyp < 0.f;
        return make_float2(flip ? -f.z : f.z, flip ? -f.w : f.w);
    }
    const float nx = cd.nx / R, ny = cd.ny / R;
    return make_float2(f.x * nx + f.z * ny, f.y * nx + f.w * ny);
}

// the ray against body b's own shape (after the candidate test): tin alone
template <int CAPS>
__device__ __forceinline__ bool q_ray_body(unsigned kind, const QRay& r, float4 m, float4 f, float2 h, float& tin, const PolyRec* poly)
{
    if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) { int edge; return q_ray_polygon(r, m, f, poly, tin, edge); }
    if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) {
        QCastDisc cd;
        const bool hit = q_ray_capsule(r.ox - m.z, r.oy - m.w, r.dx, r.dy, r.max_t, f, h.x - h.y, h.y, cd);
        tin = cd.tin;
        return hit;
    }
    if (kind != 0u) { float nx, ny; return q_ray_circle(r, m, h.x, tin, nx, ny); }
    QRayBox rb;
    const bool hit = q_ray_box(r, m, f, h, rb);
    tin = rb.tin;
    return hit;
}

// ---- the shape predicates (include/phyx_amd.h: oriented boxes and box casts) -------------------------------------------------------------
__device__ __forceinline__ float2 q_box_extents(const QBox& q)
{
    return make_float2(fabsf(q.xx) * q.hx + fabsf(q.yx) * q.hy, fabsf(q.xy) * q.hx + fabsf(q.yy) * q.hy);
}

// axis k of the four, in the header's order: X, Y, xv, yv
__device__ __forceinline__ float2 q_box_axis_of(const QBox& q, float4 f, int k)
{
    return k == 0 ? make_float2(q.xx, q.xy) : k == 1 ? make_float2(q.yx, q.yy) : k == 2 ? make_float2(f.x, f.y) : make_float2(f.z, f.w);
}

// one axis A, the same expression for all four: s = the centres' distance along A, R = the two boxes' radii along A
__device__ __forceinline__ void q_box_axis(const QBox& q, float cx, float cy, float4 f, float2 h, float2 A, float& s, float& R)
{
    s = cx * A.x + cy * A.y;
    const float rq = fabsf(q.xx * A.x + q.xy * A.y) * q.hx + fabsf(q.yx * A.x + q.yy * A.y) * q.hy;
    const float rb = fabsf(f.x * A.x + f.y * A.y) * h.x + fabsf(f.z * A.x + f.w * A.y) * h.y;
    R = rq + rb;
}

// the AABB conjunct (a body's AABB or a node's bounds, widened by the query's extents e)
__device__ __forceinline__ bool q_box_near(const QBox& q, float2 e, float4 a)
{
    return a.x - e.x <= q.px && a.z + e.x >= q.px && a.y - e.y <= q.py && a.w + e.y >= q.py;
}

__device__ __forceinline__ bool q_box_overlap(const QBox& q, float2 e, float4 a, float4 m, float4 f, float2 h)
{
    if (!q_box_near(q, e, a)) return false;
    const float cx = q.px - m.z, cy = q.py - m.w;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float s, R;
        q_box_axis(q, cx, cy, f, h, q_box_axis_of(q, f, k), s, R);
        in = in && fabsf(s) <= R;
    }
    return in;
}

// candidate test of a cast against an AABB (a body's or a node's bounds): the ray's test on the bounds widened by e
__device__ __forceinline__ bool q_cast_aabb(const QCast& c, float2 e, float4 a)
{
    if (!(a.x <= a.z && a.y <= a.w)) return false;
    float tin; bool xe;
    return q_ray_test(c.b.px, c.b.py, c.dx, c.dy, a.x - e.x, a.y - e.y, a.z + e.x, a.w + e.y, c.max_t, tin, xe);
}

struct QCastBox { float tin, v; int axis; };      // v: the direction along the entering axis

// the four slabs (after the candidate test); the entering axis is the first that attains tin
__device__ __forceinline__ bool q_cast_box(const QCast& c, float4 m, float4 f, float2 h, QCastBox& out)
{
    const float cx = c.b.px - m.z, cy = c.b.py - m.w;
    bool ok = true;
    float tout = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 A = q_box_axis_of(c.b, f, k);
        float s, R, t0, t1;
        q_box_axis(c.b, cx, cy, f, h, A, s, R);
        const float v = c.dx * A.x + c.dy * A.y;
        ok = q_slab(s, v, -R, R, t0, t1) && ok;
        if (k == 0 || t0 > out.tin) { out.tin = t0; out.v = v; out.axis = k; }
        if (k == 0 || t1 < tout) tout = t1;
    }
    return ok && out.tin <= tout && tout >= 0.f && out.tin <= c.max_t;
}

// ---- the round predicates (include/phyx_amd.h: circles and circle casts) ------------------------------------------------------------------
// the AABB conjunct (a body's AABB or a node's bounds, widened by the radius): q_box_near with the extents (r, r)
__device__ __forceinline__ bool q_disc_near(const QDisc& c, float4 a)
{
    return a.x - c.r <= c.cx && a.z + c.r >= c.cx && a.y - c.r <= c.cy && a.w + c.r >= c.cy;
}

// the circle against body b's own shape: the centre's offset from the closest point of the box, or the two radii's sum
template <int CAPS>
__device__ __forceinline__ bool q_disc_overlap(const QDisc& c, float4 a, unsigned kind, float4 m, float4 f, float2 h)
{
    if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) kind = 0u;      // (a polygon is its frame box here)
    if (!q_disc_near(c, a)) return false;
    const float ex = c.cx - m.z, ey = c.cy - m.w;
    if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) {
        const float u = ex * f.x + ey * f.y, v = ex * f.z + ey * f.w;
        const float R = c.r + h.y, gx = u - q_clamp(u, h.x - h.y);
        return gx * gx + v * v <= R * R;
    }
    if (kind != 0u) { const float R = c.r + h.x; return ex * ex + ey * ey <= R * R; }
    const float u = ex * f.x + ey * f.y, v = ex * f.z + ey * f.w;
    const float qu = u < -h.x ? -h.x : (u > h.x ? h.x : u), qv = v < -h.y ? -h.y : (v > h.y ? h.y : v);
    const float gx = u - qu, gy = v - qv;
    return gx * gx + gy * gy <= c.r * c.r;
}

// candidate test of a circle cast against an AABB (a body's or a node's bounds): q_cast_aabb with the extents (r, r)
__device__ __forceinline__ bool q_cast_aabb(const QDiscCast& c, float4 a)
{
    if (!(a.x <= a.z && a.y <= a.w)) return false;
    float tin; bool xe;
    return q_ray_test(c.c.cx, c.c.cy, c.dx, c.dy, a.x - c.c.r, a.y - c.c.r, a.z + c.c.r, a.w + c.c.r, c.max_t, tin, xe);
}

// the centre's ray against the body widened by the radius (after the candidate test): a circle body is the disc of radius r + rb, a
// capsule body the capsule of radius r + rb (q_ray_capsule); a box is the union of six convex parts, each met by its own rule, and the earliest entry wins (the first part in order on a tie).
// Every part is evaluated and the winner kept by selects on named values: no run-time-indexed array (narrowphase.h).
template <int CAPS>
__device__ __forceinline__ bool q_cast_disc(const QDiscCast& c, unsigned kind, float4 m, float4 f, float2 h, QCastDisc& out)
{
    if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) kind = 0u;      // (a polygon is its frame box here)
    out.tin = 0.f; out.part = 0; out.ox = 0.f; out.oy = 0.f; out.dxp = 0.f; out.dyp = 0.f; out.nx = 0.f; out.ny = 0.f;
    const float rx = c.c.cx - m.z, ry = c.c.cy - m.w;
    if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) return q_ray_capsule(rx, ry, c.dx, c.dy, c.max_t, f, h.x - h.y, c.c.r + h.y, out);
    if (kind != 0u) {
        out.part = Q_PART_BODY;
        return q_ray_disc(rx, ry, c.dx, c.dy, c.max_t, c.c.r + h.x, out.tin, out.nx, out.ny);
    }
    const float ox = rx * f.x + ry * f.y, oy = rx * f.z + ry * f.w;
    out.ox = ox; out.oy = oy;
    out.dxp = c.dx * f.x + c.dy * f.y;
    out.dyp = c.dx * f.z + c.dy * f.w;
    const float wx = h.x + c.c.r, wy = h.y + c.c.r;
    float tin = 0.f;
    bool xe = false;
    bool hit = q_ray_test(ox, oy, out.dxp, out.dyp, -wx, -h.y, wx, h.y, c.max_t, tin, xe);
    out.tin = hit ? tin : 0.f;
    {
        const bool pass = q_ray_test(ox, oy, out.dxp, out.dyp, -h.x, -wy, h.x, wy, c.max_t, tin, xe);
        const bool better = pass && (!hit || tin < out.tin);
        out.tin = better ? tin : out.tin; out.part = better ? 1 : out.part;
        hit = hit || pass;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float kx = (k & 1) ? h.x : -h.x, ky = (k & 2) ? h.y : -h.y;
        float nx, ny;
        const bool pass = q_ray_disc(ox - kx, oy - ky, out.dxp, out.dyp, c.max_t, c.c.r, tin, nx, ny);
        const bool better = pass && (!hit || tin < out.tin);
        out.tin = better ? tin : out.tin; out.part = better ? 2 + k : out.part;
        out.nx = better ? nx : out.nx; out.ny = better ? ny : out.ny;
        hit = hit || pass;
    }
    return hit;
}

// a circle cast's normal from what q_cast_disc left of the winner (tin >= 0; r: the cast circle's radius): the circle casts' finish and
// the continuous bodies' pass (sweep_kernels.h) both take it from here
template <int CAPS>
__device__ __forceinline__ float2 q_cast_disc_normal(const QCastDisc& cd, float4 f, float2 sz, float r)
{
    if (CAPS && cd.part >= Q_PART_SIDE) return q_capsule_normal(cd, f, r + sz.y);
    if (cd.part < 2) {                                                      // a face, by where the centre is at the entry: an exact copy
        const float px = cd.ox + cd.tin * cd.dxp, py = cd.oy + cd.tin * cd.dyp;
        const bool xface = fabsf(px) - sz.x >= fabsf(py) - sz.y;
        const float nx = xface ? f.x : f.z, ny = xface ? f.y : f.w;
        const bool flip = (xface ? px : py) < 0.f;
        return make_float2(flip ? -nx : nx, flip ? -ny : ny);
    }
    if (cd.part == Q_PART_BODY) { const float R = r + sz.x; return make_float2(cd.nx / R, cd.ny / R); }
    const float nx = cd.nx / r, ny = cd.ny / r;                             // a corner: the local normal through the frame
    return make_float2(f.x * nx + f.z * ny, f.y * nx + f.w * ny);
}

__device__ __forceinline__ unsigned long long q_ray_key(float tin, int body)
{
    const float t = tin > 0.f ? tin : 0.f;                       // t >= 0: its bits order like its value
    return ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)body;
}

// an unsigned key that orders like the float (the index build's bounds of the centres; the nearest query's distances, which may be negative)
__device__ __forceinline__ unsigned q_fkey(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float q_funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// ---- the nearest-body predicates (include/phyx_amd.h: phx_world_query_nearest; tests/near_spec.py) ------------------------------------------
// what body b is to the point p: the signed distance (negative inside), the outward normal there and the surface point
struct QNear { float sd, nx, ny, px, py; };

// (gx / l, gy / l); a length of 0 gives (0, 0)
__device__ __forceinline__ float2 q_unit(float gx, float gy, float l) { return l > 0.f ? make_float2(gx / l, gy / l) : make_float2(0.f, 0.f); }

// Each kind by its closed form, with e = p - pos and (u, v) its frame coordinates: the box by the clamp of q_disc_overlap (inside: the
// face of the smaller depth, x on a tie), the circle by its centre, the capsule by the qu clamp, the polygon by the region selection of
// the disc / polygon candidate rule (narrowphase.h).  A stored face normal is an exact copy; a corner's, a vertex's or a round body's
// goes through the frame.  The scan and the tree read .sd alone (the rest is dead code there); k_qnear_finish reads the rest.
template <int CAPS>
__device__ __forceinline__ QNear q_near_body(unsigned kind, float4 m, float4 f, float2 h, const PolyRec* __restrict__ poly, float x, float y)
{
    const float ex = x - m.z, ey = y - m.w;
    const float u = ex * f.x + ey * f.y, v = ex * f.z + ey * f.w;
    QNear o;
    if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) {
        const int n = poly->count;
        int k = 0;
        float s = 0.f;
        for (int j = 0; j < n; ++j) {
            const float d = poly->n[2 * j] * (u - poly->v[2 * j]) + poly->n[2 * j + 1] * (v - poly->v[2 * j + 1]);
            if (j == 0 || d > s) { s = d; k = j; }
        }
        const float vkx = poly->v[2 * k], vky = poly->v[2 * k + 1];
        if (s > 0.f) {
            const int k1 = k + 1 < n ? k + 1 : 0;
            const float vnx = poly->v[2 * k1], vny = poly->v[2 * k1 + 1];
            const float e0 = vnx - vkx, e1 = vny - vky;
            const float t = (u - vkx) * e0 + (v - vky) * e1, ee = e0 * e0 + e1 * e1;
            const bool lo = t < 0.f, hi = !lo && t > ee;
            if (lo || hi) {
                const float qx = lo ? vkx : vnx, qy = lo ? vky : vny;
                const float gx = u - qx, gy = v - qy;
                o.sd = sqrtf(gx * gx + gy * gy);
                const float2 l = q_unit(gx, gy, o.sd);
                o.nx = f.x * l.x + f.z * l.y; o.ny = f.y * l.x + f.w * l.y;
                o.px = (m.z + f.x * qx) + f.z * qy; o.py = (m.w + f.y * qx) + f.w * qy;
                return o;
            }
        }
        const float nx = poly->n[2 * k], ny = poly->n[2 * k + 1];
        o.sd = s;
        o.nx = f.x * nx + f.z * ny; o.ny = f.y * nx + f.w * ny;
        o.px = x - o.nx * s; o.py = y - o.ny * s;
        return o;
    }
    if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) {
        const float r = h.y, qu = q_clamp(u, h.x - h.y), gx = u - qu;
        const float len = sqrtf(gx * gx + v * v);
        const float2 l = q_unit(gx, v, len);
        o.sd = len - r;
        o.nx = f.x * l.x + f.z * l.y; o.ny = f.y * l.x + f.w * l.y;
        o.px = (m.z + f.x * qu) + o.nx * r; o.py = (m.w + f.y * qu) + o.ny * r;
        return o;
    }
    if (kind != 0u) {
        const float len = sqrtf(ex * ex + ey * ey);
        const float2 l = q_unit(ex, ey, len);
        o.sd = len - h.x;
        o.nx = l.x; o.ny = l.y;
        o.px = m.z + l.x * h.x; o.py = m.w + l.y * h.x;
        return o;
    }
    const float ax = fabsf(u) - h.x, ay = fabsf(v) - h.y;
    if (ax <= 0.f && ay <= 0.f) {
        const bool xface = ax >= ay, flip = (xface ? u : v) < 0.f;
        const float nx = xface ? f.x : f.z, ny = xface ? f.y : f.w;
        o.sd = xface ? ax : ay;
        o.nx = flip ? -nx : nx; o.ny = flip ? -ny : ny;
        o.px = x - o.nx * o.sd; o.py = y - o.ny * o.sd;
        return o;
    }
    const float qu = q_clamp(u, h.x), qv = q_clamp(v, h.y);
    const float gx = u - qu, gy = v - qv;
    o.sd = sqrtf(gx * gx + gy * gy);
    if (gy == 0.f) { const bool flip = u < 0.f; o.nx = flip ? -f.x : f.x; o.ny = flip ? -f.y : f.y; }              // a face region: x first
    else if (gx == 0.f) { const bool flip = v < 0.f; o.nx = flip ? -f.z : f.z; o.ny = flip ? -f.w : f.w; }
    else { const float2 l = q_unit(gx, gy, o.sd); o.nx = f.x * l.x + f.z * l.y; o.ny = f.y * l.x + f.w * l.y; }
    o.px = (m.z + f.x * qu) + f.z * qv; o.py = (m.w + f.y * qu) + f.w * qv;
    return o;
}

// la: the point's distance from an AABB (a body's or a node's bounds), 0 inside
__device__ __forceinline__ float q_near_gap(float4 a, float x, float y)
{
    const float gx = fmaxf(fmaxf(a.x - x, x - a.z), 0.f), gy = fmaxf(fmaxf(a.y - y, y - a.w), 0.f);
    return sqrtf(gx * gx + gy * gy);
}

// D = (la > 0 ? max(sd, la) : sd), never -0.  The fp32 sd may fall a rounding short of la; with the max D >= la holds bit for bit, and la
// is monotone in the box: a node whose la exceeds the best D so far holds no body that can win or tie (k_qtree, QK_NEAR).
__device__ __forceinline__ float q_near_distance(float sd, float la)
{
    const float d = la > 0.f ? (sd >= la ? sd : la) : sd;
    return d == 0.f ? 0.f : d;
}

// a nearest query {p, max_dist} travels as a QDisc {p, r = max_dist}: max_dist == 0 is valid
__device__ __forceinline__ bool q_near_ok(const QDisc& c) { return isfinite(c.cx) && isfinite(c.cy) && isfinite(c.r) && c.r >= 0.f; }

// (q_fkey(D) << 32) | body of a candidate, ~0 of any other body: the smallest key is the smallest D, ties to the lowest body index
template <int CAPS>
__device__ __forceinline__ unsigned long long q_near_key(const QDisc& c, float4 a, unsigned kind, float4 m, float4 f, float2 h, const PolyRec* __restrict__ poly, int body)
{
    if (!(a.x <= a.z && a.y <= a.w) || !q_disc_near(c, a)) return ~0ull;
    const float D = q_near_distance(q_near_body<CAPS>(kind, m, f, h, poly, c.cx, c.cy).sd, q_near_gap(a, c.cx, c.cy));
    return D <= c.r ? ((unsigned long long)q_fkey(D) << 32) | (unsigned)body : ~0ull;
}

__device__ __forceinline__ bool q_point_ok(float px, float py) { return isfinite(px) && isfinite(py); }
__device__ __forceinline__ bool q_ray_ok(const QRay& r)
{
    return isfinite(r.ox) && isfinite(r.oy) && isfinite(r.dx) && isfinite(r.dy) && isfinite(r.max_t) && r.max_t >= 0.f && (r.dx != 0.f || r.dy != 0.f);
}
__device__ __forceinline__ bool q_box_ok(float4 q) { return isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w); }

__device__ __forceinline__ bool q_shape_ok(const QBox& q)
{
    return isfinite(q.px) && isfinite(q.py) && isfinite(q.xx) && isfinite(q.xy) && isfinite(q.yx) && isfinite(q.yy) && isfinite(q.hx) && isfinite(q.hy) &&
           q.hx > 0.f && q.hy > 0.f;
}
__device__ __forceinline__ bool q_cast_ok(const QCast& c)
{
    return q_shape_ok(c.b) && isfinite(c.dx) && isfinite(c.dy) && isfinite(c.max_t) && c.max_t >= 0.f && (c.dx != 0.f || c.dy != 0.f);
}

__device__ __forceinline__ bool q_disc_ok(const QDisc& c) { return isfinite(c.cx) && isfinite(c.cy) && isfinite(c.r) && c.r > 0.f; }
__device__ __forceinline__ bool q_cast_ok(const QDiscCast& c)
{
    return q_disc_ok(c.c) && isfinite(c.dx) && isfinite(c.dy) && isfinite(c.max_t) && c.max_t >= 0.f && (c.dx != 0.f || c.dy != 0.f);
}

__device__ __forceinline__ QRay q_load_ray(const float* __restrict__ rays, int q)
{
    const float* p = rays + 5 * (size_t)q;
    return QRay{p[0], p[1], p[2], p[3], p[4]};
}

__device__ __forceinline__ QBox q_load_box(const float* __restrict__ p) { return QBox{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}; }
__device__ __forceinline__ QCast q_load_cast(const float* __restrict__ casts, int q)
{
    const float* p = casts + 11 * (size_t)q;
    return QCast{q_load_box(p), p[8], p[9], p[10]};
}

__device__ __forceinline__ QDisc q_load_disc(const float* __restrict__ p) { return QDisc{p[0], p[1], p[2]}; }
__device__ __forceinline__ QDiscCast q_load_disc_cast(const float* __restrict__ casts, int q)
{
    const float* p = casts + 6 * (size_t)q;
    return QDiscCast{q_load_disc(p), p[3], p[4], p[5]};
}

__device__ __forceinline__ unsigned long long q_lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

__device__ __forceinline__ unsigned long long q_wave_min64(unsigned long long v)
{
    for (int s = 32; s > 0; s >>= 1) { const unsigned long long o = __shfl_xor(v, s); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned q_wave_min(unsigned v)
{
    for (int s = 32; s > 0; s >>= 1) v = min(v, (unsigned)__shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ unsigned q_wave_sum(unsigned v)
{
    for (int s = 32; s > 0; s >>= 1) v += (unsigned)__shfl_xor(v, s);
    return v;
}

// ---- small fills ------------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_qfill_u64(unsigned long long* __restrict__ p, int n, unsigned long long v)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

// the ray results from the winners' keys: the winner's test is made again, by the same code, for its normal
template <int CAPS>
static __global__ void __launch_bounds__(256) k_qray_finish(WorldBodies w, const float* __restrict__ rays, int count,
                                                            const unsigned long long* __restrict__ keys, phx_ray_hit* __restrict__ out)
{
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < count; q += gridDim.x * blockDim.x) {
        const unsigned long long k = keys[q];
        phx_ray_hit h;
        h.body = -1; h.t = 0.f; h.normal.x = h.normal.y = 0.f; h.point.x = h.point.y = 0.f;
        if (k != ~0ull) {
            const int b = (int)(unsigned)(k & 0xFFFFFFFFull);
            const QRay r = q_load_ray(rays, q);
            const float4 m = w.s.mpos[b], f = w.frame[b];
            const float2 sz = w.size[b];
            float t;
            const unsigned kind = q_kind<CAPS>(w.kinds, b);
            if (CAPS == 2 && kind == (unsigned)PHX_SHAPE_POLYGON) {
                const PolyRec* poly = q_poly<CAPS>(w, b);
                float tin; int edge;
                (void)q_ray_polygon(r, m, f, poly, tin, edge);
                t = tin > 0.f ? tin : 0.f;
                if (!(tin < 0.f) && edge >= 0) {
                    const float nx = poly->n[2 * edge], ny = poly->n[2 * edge + 1];
                    h.normal.x = f.x * nx + f.z * ny; h.normal.y = f.y * nx + f.w * ny;
                }
            } else if (CAPS && kind == (unsigned)PHX_SHAPE_CAPSULE) {
                QCastDisc cd;
                (void)q_ray_capsule(r.ox - m.z, r.oy - m.w, r.dx, r.dy, r.max_t, f, sz.x - sz.y, sz.y, cd);
                t = cd.tin > 0.f ? cd.tin : 0.f;
                if (!(cd.tin < 0.f)) { const float2 nn = q_capsule_normal(cd, f, sz.y); h.normal.x = nn.x; h.normal.y = nn.y; }
            } else if (kind != 0u) {
                float tin, nx, ny;
                (void)q_ray_circle(r, m, sz.x, tin, nx, ny);
                t = tin > 0.f ? tin : 0.f;
                if (!(tin < 0.f)) { h.normal.x = nx / sz.x; h.normal.y = ny / sz.x; }
            } else {
                QRayBox rb;
                (void)q_ray_box(r, m, f, sz, rb);
                t = rb.tin > 0.f ? rb.tin : 0.f;
                if (!(rb.tin < 0.f)) {
                    const float nx = rb.xenter ? f.x : f.z, ny = rb.xenter ? f.y : f.w;
                    const bool flip = (rb.xenter ? rb.dxp : rb.dyp) > 0.f;
                    h.normal.x = flip ? -nx : nx; h.normal.y = flip ? -ny : ny;
                }
            }
            h.body = b; h.t = t;
            h.point.x = r.ox + t * r.dx;
            h.point.y = r.oy + t * r.dy;
        }
        out[q] = h;
    }
}

// the cast results from the winners' keys, as k_qray_finish (SHAPE: QSHAPE_BOX box casts, QSHAPE_DISC circle casts)
template <int SHAPE, int CAPS>
static __global__ void __launch_bounds__(256) k_qcast_finish(WorldBodies w, const float* __restrict__ casts, int count,
                                                             const unsigned long long* __restrict__ keys, phx_shape_hit* __restrict__ out)
{
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < count; q += gridDim.x * blockDim.x) {
        const unsigned long long k = keys[q];
        phx_shape_hit h;
        h.body = -1; h.t = 0.f; h.normal.x = h.normal.y = 0.f;
        if (k != ~0ull && SHAPE == QSHAPE_DISC) {
            const int b = (int)(unsigned)(k & 0xFFFFFFFFull);
            const QDiscCast c = q_load_disc_cast(casts, q);
            const float4 f = w.frame[b];
            const float2 sz = w.size[b];
            QCastDisc cd;
            (void)q_cast_disc<CAPS>(c, q_kind<CAPS>(w.kinds, b), w.s.mpos[b], f, sz, cd);
            h.body = b; h.t = cd.tin > 0.f ? cd.tin : 0.f;
            if (!(cd.tin < 0.f)) { const float2 nn = q_cast_disc_normal<CAPS>(cd, f, sz, c.c.r); h.normal.x = nn.x; h.normal.y = nn.y; }
        } else if (k != ~0ull) {
            const int b = (int)(unsigned)(k & 0xFFFFFFFFull);
            const QCast c = q_load_cast(casts, q);
            const float4 f = w.frame[b];
            QCastBox cb;
            (void)q_cast_box(c, w.s.mpos[b], f, w.size[b], cb);
            h.body = b; h.t = cb.tin > 0.f ? cb.tin : 0.f;
            if (!(cb.tin < 0.f)) {
                const float2 n = q_box_axis_of(c.b, f, cb.axis);
                h.normal.x = cb.v > 0.f ? -n.x : n.x; h.normal.y = cb.v > 0.f ? -n.y : n.y;
            }
        }
        out[q] = h;
    }
}

// the nearest results from the winners' keys: the distance is the key's, the winner's normal and point are made again by the same code
template <int CAPS>
static __global__ void __launch_bounds__(256) k_qnear_finish(WorldBodies w, const float* __restrict__ queries, int count,
                                                             const unsigned long long* __restrict__ keys, phx_near_hit* __restrict__ out)
{
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < count; q += gridDim.x * blockDim.x) {
        const unsigned long long k = keys[q];
        phx_near_hit h;
        h.body = -1; h.distance = 0.f; h.normal.x = h.normal.y = 0.f; h.point.x = h.point.y = 0.f;
        if (k != ~0ull) {
            const int b = (int)(unsigned)(k & 0xFFFFFFFFull);
            const QDisc c = q_load_disc(queries + 3 * (size_t)q);
            const QNear o = q_near_body<CAPS>(q_kind<CAPS>(w.kinds, b), w.s.mpos[b], w.frame[b], w.size[b], q_poly<CAPS>(w, b), c.cx, c.cy);
            h.body = b; h.distance = q_funkey((unsigned)(k >> 32));
            h.normal.x = o.nx; h.normal.y = o.ny;
            h.point.x = o.px; h.point.y = o.py;
        }
        out[q] = h;
    }
}

// ---- scan path --------------------------------------------------------------------------------------------------------------------
// blockIdx.y = the tile of queries [q0, q0 + Q_TILE); bodies grid-strided in lanes.  out: 0xFFFFFFFF (= -1) where nothing was found.
template <int CAPS>
static __global__ void __launch_bounds__(256) k_qscan_points(WorldBodies w, int n, const float* __restrict__ pts, int count, int q0, int flags,
                                                             unsigned* __restrict__ out)
{
    __shared__ float2 qp[Q_TILE];
    __shared__ int qok[Q_TILE];
    const int base_q = q0 + blockIdx.y * Q_TILE, nq = min(Q_TILE, count - base_q);
    if ((int)threadIdx.x < nq) {
        const float px = pts[2 * (size_t)(base_q + threadIdx.x)], py = pts[2 * (size_t)(base_q + threadIdx.x) + 1];
        qp[threadIdx.x] = make_float2(px, py);
        qok[threadIdx.x] = q_point_ok(px, py);
    }
    __syncthreads();
    const bool skip = (flags & Q_SKIP_STATIC) != 0;
    for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform trip count: the ballots below)
        const int i = base + threadIdx.x;
        const bool live = i < n;
        float4 a = make_float4(NAN, NAN, NAN, NAN), m = make_float4(0.f, 0.f, 0.f, 0.f), f = m;
        float2 h = make_float2(0.f, 0.f);
        if (live) { a = w.aabb[i]; m = w.s.mpos[i]; f = w.frame[i]; h = w.size[i]; }
        const bool any = live && !(skip && q_static(m, w.sleep, i));
        const unsigned round = live ? q_kind<CAPS>(w.kinds, i) : 0u;
        for (int q = 0; q < nq; ++q) {
            const float2 p = qp[q];
            const bool hit = any && qok[q] && q_point_in_body<CAPS>(round, a, m, f, h, p.x, p.y, q_poly<CAPS>(w, i));
            const unsigned long long mask = __ballot(hit);
            if (mask && (int)(threadIdx.x & 63) == __builtin_ctzll(mask)) atomicMin(&out[base_q + q], (unsigned)i);      // (the lowest lane holds the lowest body)
        }
    }
}

// SHAPE: rays (5 floats per query), box casts (11) or circle casts (6)
template <int SHAPE, int CAPS>
static __global__ void __launch_bounds__(256) k_qscan_rays(WorldBodies w, int n, const float* __restrict__ rays, int count, int q0, int flags,
                                                           unsigned long long* __restrict__ keys)
{
    __shared__ QRay qr[Q_TILE];
    __shared__ QCast qc[Q_TILE];
    __shared__ QDiscCast qd[Q_TILE];
    __shared__ float2 qe[Q_TILE];
    __shared__ int qok[Q_TILE];
    constexpr bool CAST = SHAPE == QSHAPE_BOX, DISC = SHAPE == QSHAPE_DISC;
    const int base_q = q0 + blockIdx.y * Q_TILE, nq = min(Q_TILE, count - base_q);
    if ((int)threadIdx.x < nq) {
        if (CAST) {
            const QCast c = q_load_cast(rays, base_q + threadIdx.x);
            qc[threadIdx.x] = c;
            qe[threadIdx.x] = q_box_extents(c.b);
            qok[threadIdx.x] = q_cast_ok(c);
        } else if (DISC) {
            const QDiscCast c = q_load_disc_cast(rays, base_q + threadIdx.x);
            qd[threadIdx.x] = c;
            qok[threadIdx.x] = q_cast_ok(c);
        } else {
            const QRay r = q_load_ray(rays, base_q + threadIdx.x);
            qr[threadIdx.x] = r;
            qok[threadIdx.x] = q_ray_ok(r);
        }
    }
    __syncthreads();
    const bool skip = (flags & Q_SKIP_STATIC) != 0;
    for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const int i = base + threadIdx.x;
        const bool live = i < n;
        float4 a = make_float4(NAN, NAN, NAN, NAN), m = make_float4(0.f, 0.f, 0.f, 0.f), f = m;
        float2 h = make_float2(0.f, 0.f);
        if (live) { a = w.aabb[i]; m = w.s.mpos[i]; f = w.frame[i]; h = w.size[i]; }
        const bool any = live && !(skip && q_static(m, w.sleep, i));
        const unsigned round = !CAST && live ? q_kind<CAPS>(w.kinds, i) : 0u;
        for (int q = 0; q < nq; ++q) {
            bool hit;
            float tin;
            if (CAST) {
                const QCast c = qc[q];
                QCastBox cb;
                hit = any && qok[q] && q_cast_aabb(c, qe[q], a) && q_cast_box(c, m, f, h, cb);
                tin = hit ? cb.tin : 0.f;
            } else if (DISC) {
                const QDiscCast c = qd[q];
                QCastDisc cd;
                hit = any && qok[q] && q_cast_aabb(c, a) && q_cast_disc<CAPS>(c, round, m, f, h, cd);
                tin = hit ? cd.tin : 0.f;
            } else {
                const QRay r = qr[q];
                float t0 = 0.f;
                hit = any && qok[q] && q_ray_aabb(r, a) && q_ray_body<CAPS>(round, r, m, f, h, t0, q_poly<CAPS>(w, i));
                tin = hit ? t0 : 0.f;
            }
            if (!__ballot(hit)) continue;
            const unsigned long long k = q_wave_min64(hit ? q_ray_key(tin, i) : ~0ull);
            if ((threadIdx.x & 63) == 0) atomicMin(&keys[base_q + q], k);
        }
    }
}

// nearest queries (3 floats per query), a sibling of k_qscan_rays: the plain statement of the rule, every body against every query of the
// tile, nothing skipped by what was found so far
template <int CAPS>
static __global__ void __launch_bounds__(256) k_qscan_near(WorldBodies w, int n, const float* __restrict__ queries, int count, int q0, int flags,
                                                           unsigned long long* __restrict__ keys)
{
    __shared__ QDisc qd[Q_TILE];
    __shared__ int qok[Q_TILE];
    const int base_q = q0 + blockIdx.y * Q_TILE, nq = min(Q_TILE, count - base_q);
    if ((int)threadIdx.x < nq) {
        const QDisc c = q_load_disc(queries + 3 * (size_t)(base_q + threadIdx.x));
        qd[threadIdx.x] = c;
        qok[threadIdx.x] = q_near_ok(c);
    }
    __syncthreads();
    const bool skip = (flags & Q_SKIP_STATIC) != 0;
    for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // (uniform trip count: the ballots below)
        const int i = base + threadIdx.x;
        const bool live = i < n;
        float4 a = make_float4(NAN, NAN, NAN, NAN), m = make_float4(0.f, 0.f, 0.f, 0.f), f = m;
        float2 h = make_float2(0.f, 0.f);
        if (live) { a = w.aabb[i]; m = w.s.mpos[i]; f = w.frame[i]; h = w.size[i]; }
        const bool any = live && !(skip && q_static(m, w.sleep, i));
        const unsigned kind = live ? q_kind<CAPS>(w.kinds, i) : 0u;
        for (int q = 0; q < nq; ++q) {
            unsigned long long k = ~0ull;
            if (any && qok[q]) k = q_near_key<CAPS>(qd[q], a, kind, m, f, h, q_poly<CAPS>(w, i), i);
            if (!__ballot(k != ~0ull)) continue;
            k = q_wave_min64(k);
            if ((threadIdx.x & 63) == 0) atomicMin(&keys[base_q + q], k);
        }
    }
}

// AABB queries (SHAPE: oriented-box queries, 8 floats per query, or circle queries, 3), one workgroup per 256 consecutive bodies (blockIdx.x = body block of
// `bblocks`), blockIdx.y = tile.
//   QS_COUNT    writes the hit count of every (query, body block) to table[(q - q0) * bblocks + block] (query-major: its exclusive scan
//               places the blocks' hits of a query one after the other, in body order) and adds it to qcount[q];
//   QS_RECOUNT  the table alone (a later chunk of queries counted again: the table holds one chunk);
//   QS_FILL     writes the hits at base + table[...] + rank.
enum { QS_COUNT = 0, QS_RECOUNT = 1, QS_FILL = 2 };
template <int MODE, int SHAPE, int CAPS>
static __global__ void __launch_bounds__(256) k_qscan_aabb(WorldBodies w, int n, const float* __restrict__ boxes, int count, int q0, int flags, int bblocks,
                                                           unsigned* __restrict__ table, unsigned* __restrict__ qcount, unsigned base, int* __restrict__ hits)
{
    __shared__ float4 qb[Q_TILE];
    __shared__ QBox qo[Q_TILE];
    __shared__ QDisc qd[Q_TILE];
    __shared__ float2 qe[Q_TILE];
    __shared__ int qok[Q_TILE];
    __shared__ unsigned long long masks[Q_TILE][4];
    constexpr bool OBB = SHAPE == QSHAPE_BOX, DISC = SHAPE == QSHAPE_DISC;
    const int tile_q = blockIdx.y * Q_TILE, base_q = q0 + tile_q, nq = min(Q_TILE, count - base_q);
    if ((int)threadIdx.x < nq) {
        if (OBB) {
            const QBox q = q_load_box(boxes + 8 * (size_t)(base_q + threadIdx.x));
            qo[threadIdx.x] = q;
            qe[threadIdx.x] = q_box_extents(q);
            qok[threadIdx.x] = q_shape_ok(q);
        } else if (DISC) {
            const QDisc q = q_load_disc(boxes + 3 * (size_t)(base_q + threadIdx.x));
            qd[threadIdx.x] = q;
            qok[threadIdx.x] = q_disc_ok(q);
        } else {
            const float* p = boxes + 4 * (size_t)(base_q + threadIdx.x);
            const float4 q = make_float4(p[0], p[1], p[2], p[3]);
            qb[threadIdx.x] = q;
            qok[threadIdx.x] = q_box_ok(q);
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const float4 a = live ? w.aabb[i] : make_float4(NAN, NAN, NAN, NAN);
    const float4 m = (OBB || DISC || (flags & Q_SKIP_STATIC)) ? w.s.mpos[live ? i : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool any = live && !((flags & Q_SKIP_STATIC) && q_static(m, w.sleep, i));
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 h = make_float2(0.f, 0.f);
    if ((OBB || DISC) && live) { f = w.frame[i]; h = w.size[i]; }
    const unsigned round = DISC && live ? q_kind<CAPS>(w.kinds, i) : 0u;
    unsigned long long mine = 0;
    for (int q = 0; q < nq; ++q) {
        const bool hit = any && qok[q] && (OBB ? q_box_overlap(qo[q], qe[q], a, m, f, h) : DISC ? q_disc_overlap<CAPS>(qd[q], a, round, m, f, h) : q_overlap(a, qb[q]));
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) masks[q][wave] = mask;
        mine |= (unsigned long long)hit << q;
    }
    __syncthreads();
    if (MODE != QS_FILL) {
        if ((int)threadIdx.x < nq) {
            const unsigned c = (unsigned)(__popcll(masks[threadIdx.x][0]) + __popcll(masks[threadIdx.x][1]) + __popcll(masks[threadIdx.x][2]) + __popcll(masks[threadIdx.x][3]));
            table[(size_t)(tile_q + threadIdx.x) * bblocks + blockIdx.x] = c;
            if (MODE == QS_COUNT && c) atomicAdd(&qcount[base_q + threadIdx.x], c);
        }
        return;
    }
    while (mine) {
        const int q = __builtin_ctzll(mine);
        mine &= mine - 1;
        unsigned pos = base + table[(size_t)(tile_q + q) * bblocks + blockIdx.x] + (unsigned)__popcll(masks[q][wave] & q_lanes_below());
        for (int v = 0; v < wave; ++v) pos += (unsigned)__popcll(masks[q][v]);
        hits[pos] = i;
    }
}

// ---- index path: build ------------------------------------------------------------------------------------------------------------
// bounds of the AABB centres (bounds = {min x, min y, max x, max y} as order keys; NaN centres left out)
static __global__ void __launch_bounds__(256) k_qcentre_bounds(const float4* __restrict__ aabb, int n, unsigned* __restrict__ bounds)
{
    unsigned lx = 0xFFFFFFFFu, ly = 0xFFFFFFFFu, hx = 0u, hy = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = aabb[i];
        const float cx = (a.x + a.z) * 0.5f, cy = (a.y + a.w) * 0.5f;
        if (!(cx == cx) || !(cy == cy)) continue;
        const unsigned kx = q_fkey(cx), ky = q_fkey(cy);
        lx = min(lx, kx); ly = min(ly, ky); hx = max(hx, kx); hy = max(hy, ky);
    }
    lx = q_wave_min(lx); ly = q_wave_min(ly);
    for (int s = 32; s > 0; s >>= 1) { hx = max(hx, (unsigned)__shfl_xor(hx, s)); hy = max(hy, (unsigned)__shfl_xor(hy, s)); }
    if ((threadIdx.x & 63) == 0 && lx != 0xFFFFFFFFu) { atomicMin(&bounds[0], lx); atomicMin(&bounds[1], ly); atomicMax(&bounds[2], hx); atomicMax(&bounds[3], hy); }
}

__device__ __forceinline__ unsigned q_spread16(unsigned v)
{
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

__device__ __forceinline__ unsigned q_quantise(float c, float lo, float hi)
{
    const float span = hi - lo;
    if (!(span > 0.f)) return 0u;
    const float s = (c - lo) / span * 65535.f;
    return s <= 0.f ? 0u : s >= 65535.f ? 65535u : (unsigned)s;
}

// 32-bit Morton keys of the quantised centres (NaN centres: 0xFFFFFFFF, at the end); vals = the body index
static __global__ void __launch_bounds__(256) k_qmorton(const float4* __restrict__ aabb, int n, const unsigned* __restrict__ bounds,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ vals)
{
    const bool none = bounds[0] == 0xFFFFFFFFu;
    const float lx = none ? 0.f : q_funkey(bounds[0]), ly = none ? 0.f : q_funkey(bounds[1]);
    const float hx = none ? 0.f : q_funkey(bounds[2]), hy = none ? 0.f : q_funkey(bounds[3]);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = aabb[i];
        const float cx = (a.x + a.z) * 0.5f, cy = (a.y + a.w) * 0.5f;
        keys[i] = (!(cx == cx) || !(cy == cy)) ? 0xFFFFFFFFu : (q_spread16(q_quantise(cx, lx, hx)) | (q_spread16(q_quantise(cy, ly, hy)) << 1));
        vals[i] = (unsigned)i;
    }
}

// one wave per node: the exact union of its (up to) 64 children — bodies through perm (level 1) or the nodes of the level below.
// fminf / fmaxf drop a NaN operand, so a NaN AABB widens nothing; a node of nothing but NaN AABBs stays {+inf, -inf}: it passes no test.
static __global__ void __launch_bounds__(256) k_qnodes(const float4* __restrict__ src, const unsigned* __restrict__ perm, int src_cnt,
                                                       float4* __restrict__ dst, int dst_cnt)
{
    const int node = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (node >= dst_cnt) return;
    const int c = node * Q_FANOUT + lane;
    float lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    if (c < src_cnt) {
        const float4 a = src[perm ? perm[c] : (unsigned)c];
        lx = a.x; ly = a.y; hx = a.z; hy = a.w;
    }
    for (int s = 32; s > 0; s >>= 1) {
        lx = fminf(lx, __shfl_xor(lx, s)); ly = fminf(ly, __shfl_xor(ly, s));
        hx = fmaxf(hx, __shfl_xor(hx, s)); hy = fmaxf(hy, __shfl_xor(hy, s));
    }
    if (lane == 0) dst[node] = make_float4(lx, ly, hx, hy);
}

// ---- index path: traversal ----------------------------------------------------------------------------------------------------------
enum { QK_POINT = 0, QK_RAY = 1, QK_AABB_COUNT = 2, QK_AABB_FILL = 3, QK_BOX_COUNT = 4, QK_BOX_FILL = 5, QK_CAST = 6,
       QK_DISC_COUNT = 7, QK_DISC_FILL = 8, QK_DISC_CAST = 9, QK_NEAR = 10 };

// one wave per query, 4 per workgroup.  A stack entry is (level << 26) | node; a popped node's 64 children are tested by the 64 lanes,
// the passing inner nodes pushed in lane order.  Depth bound: a pop pushes at most 64 entries of the level below, so the stack never
// holds more than (levels - 1) * 63 + 64 <= Q_MAX_LEVELS * 64 entries.
//   QK_POINT       out_u32[q] = the lowest body index containing the point (0xFFFFFFFF: none)
//   QK_RAY         out_key[q] = min over hits of q_ray_key (~0: none)
//   QK_AABB_COUNT  out_u32[q] = the number of hits
//   QK_AABB_FILL   the hits at hits[seg[q] ..], in traversal order (sorted afterwards)
//   QK_BOX_COUNT, QK_BOX_FILL   the same two for oriented boxes;   QK_CAST   as QK_RAY for box casts
//   QK_DISC_COUNT, QK_DISC_FILL, QK_DISC_CAST   the same three for circles
//   QK_NEAR        out_key[q] = min over the candidates of q_near_key (~0: none).  The one kind whose walk is pruned by what it has found:
//                  the best key is reduced over the wave after every leaf, a node (when its children are tested, and again when it is
//                  popped) is skipped iff la_node > 0 && la_node > the best D so far (q_near_distance: never a change to a result), and
//                  the passing children are pushed farthest first, so that the nearest is popped next.  The other kinds' code is
//                  untouched by it: every addition sits under `if constexpr`.
// A lane tests a child's bounds with the query's AABB conjunct: the bounds widened by the box's extents or the circle's radius for the
// six kinds before QK_NEAR, by max_dist for QK_NEAR.
template <int KIND, int CAPS>
static __global__ void __launch_bounds__(256) k_qtree(WorldBodies w, QTree t, const float* __restrict__ queries, int count, int flags,
                                                      unsigned* __restrict__ out_u32, unsigned long long* __restrict__ out_key,
                                                      const unsigned* __restrict__ seg, int* __restrict__ hits)
{
    __shared__ unsigned stack_mem[4][Q_MAX_LEVELS * Q_FANOUT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool skip = (flags & Q_SKIP_STATIC) != 0;
    constexpr bool OBB = KIND == QK_BOX_COUNT || KIND == QK_BOX_FILL, DISC = KIND == QK_DISC_COUNT || KIND == QK_DISC_FILL;
    constexpr bool COUNT = KIND == QK_AABB_COUNT || KIND == QK_BOX_COUNT || KIND == QK_DISC_COUNT;
    constexpr bool FILL = KIND == QK_AABB_FILL || KIND == QK_BOX_FILL || KIND == QK_DISC_FILL;
    constexpr bool KEY = KIND == QK_RAY || KIND == QK_CAST || KIND == QK_DISC_CAST || KIND == QK_NEAR;
    for (int q = blockIdx.x * 4 + wave; q < count; q += gridDim.x * 4) {      // (the whole wave: grid-strided over the queries)
        float4 qbox = make_float4(0.f, 0.f, 0.f, 0.f);
        QRay r{0.f, 0.f, 0.f, 0.f, 0.f};
        QCast cs{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0.f, 0.f, 0.f};      // (a box query uses cs.b)
        float2 ce = make_float2(0.f, 0.f);
        QDiscCast ds{{0.f, 0.f, 0.f}, 0.f, 0.f, 0.f};                          // (a circle query uses ds.c)
        bool ok;
        if (KIND == QK_DISC_CAST) {
            ds = q_load_disc_cast(queries, q);
            ok = q_cast_ok(ds);
        } else if (KIND == QK_NEAR) {
            ds.c = q_load_disc(queries + 3 * (size_t)q);                   // ({p, max_dist})
            ok = q_near_ok(ds.c);
        } else if (DISC) {
            ds.c = q_load_disc(queries + 3 * (size_t)q);
            ok = q_disc_ok(ds.c);
        } else if (KIND == QK_POINT) {
            const float px = queries[2 * (size_t)q], py = queries[2 * (size_t)q + 1];
            ok = q_point_ok(px, py);
            qbox = make_float4(px, py, px, py);                            // (the point's closed AABB test is the overlap test with this box)
        } else if (KIND == QK_RAY) {
            r = q_load_ray(queries, q);
            ok = q_ray_ok(r);
        } else if (KIND == QK_CAST) {
            cs = q_load_cast(queries, q);
            ok = q_cast_ok(cs);
            ce = q_box_extents(cs.b);
        } else if (OBB) {
            cs.b = q_load_box(queries + 8 * (size_t)q);
            ok = q_shape_ok(cs.b);
            ce = q_box_extents(cs.b);
        } else {
            const float* p = queries + 4 * (size_t)q;
            qbox = make_float4(p[0], p[1], p[2], p[3]);
            ok = q_box_ok(qbox);
        }
        unsigned best = 0xFFFFFFFFu, n_hits = 0u, cursor = 0u;
        unsigned long long best_key = ~0ull;
        if (ok && t.levels > 0) {
            volatile unsigned* st = stack_mem[wave];
            if (lane == 0) st[0] = (unsigned)t.levels << 26;
            __builtin_amdgcn_wave_barrier();
            int sp = 1;
            while (sp > 0) {
                const unsigned e = st[--sp];
                __builtin_amdgcn_wave_barrier();
                const int level = (int)(e >> 26), node = (int)(e & ((1u << 26) - 1u));
                if constexpr (KIND == QK_NEAR) {                            // (pushed before the bound came this far down: looked at again)
                    if (best_key != ~0ull) {
                        const float la = q_near_gap(t.nodes[t.off[level] + node], ds.c.cx, ds.c.cy);
                        if (la > 0.f && la > q_funkey((unsigned)(best_key >> 32))) continue;
                    }
                }
                const int c = node * Q_FANOUT + lane;
                if (level == 1) {
                    bool hit = false;
                    int b = 0;
                    if (c < t.n) {
                        b = (int)t.perm[c];
                        const float4 a = w.aabb[b], m = w.s.mpos[b];
                        if (!(skip && q_static(m, w.sleep, b))) {
                            if (KIND == QK_POINT) hit = q_point_in_body<CAPS>(q_kind<CAPS>(w.kinds, b), a, m, w.frame[b], w.size[b], qbox.x, qbox.y, q_poly<CAPS>(w, b));
                            else if (KIND == QK_RAY) {
                                float t0 = 0.f;
                                hit = q_ray_aabb(r, a) && q_ray_body<CAPS>(q_kind<CAPS>(w.kinds, b), r, m, w.frame[b], w.size[b], t0, q_poly<CAPS>(w, b));
                                if (hit) { const unsigned long long k = q_ray_key(t0, b); best_key = k < best_key ? k : best_key; }
                            } else if (KIND == QK_CAST) {
                                QCastBox cb;
                                hit = q_cast_aabb(cs, ce, a) && q_cast_box(cs, m, w.frame[b], w.size[b], cb);
                                if (hit) { const unsigned long long k = q_ray_key(cb.tin, b); best_key = k < best_key ? k : best_key; }
                            } else if (KIND == QK_DISC_CAST) {
                                QCastDisc cd;
                                hit = q_cast_aabb(ds, a) && q_cast_disc<CAPS>(ds, q_kind<CAPS>(w.kinds, b), m, w.frame[b], w.size[b], cd);
                                if (hit) { const unsigned long long k = q_ray_key(cd.tin, b); best_key = k < best_key ? k : best_key; }
                            } else if (KIND == QK_NEAR) {
                                const unsigned long long k = q_near_key<CAPS>(ds.c, a, q_kind<CAPS>(w.kinds, b), m, w.frame[b], w.size[b], q_poly<CAPS>(w, b), b);
                                best_key = k < best_key ? k : best_key;
                            } else if (OBB) hit = q_box_overlap(cs.b, ce, a, m, w.frame[b], w.size[b]);
                            else if (DISC) hit = q_disc_overlap<CAPS>(ds.c, a, q_kind<CAPS>(w.kinds, b), m, w.frame[b], w.size[b]);
                            else hit = q_overlap(a, qbox);
                        }
                    }
                    if (KIND == QK_POINT && hit) best = min(best, (unsigned)b);
                    if (COUNT) n_hits += hit ? 1u : 0u;
                    if (FILL) {
                        const unsigned long long mask = __ballot(hit);
                        if (hit) hits[seg[q] + cursor + (unsigned)__popcll(mask & q_lanes_below())] = b;
                        cursor += (unsigned)__popcll(mask);
                    }
                    if constexpr (KIND == QK_NEAR) best_key = q_wave_min64(best_key);      // (wave-uniform: the bound every lane prunes by)
                } else {
                    bool pass = false;
                    if (c < t.cnt[level - 1]) {
                        const float4 nb = t.nodes[t.off[level - 1] + c];
                        pass = KIND == QK_RAY ? q_ray_aabb(r, nb) : KIND == QK_CAST ? q_cast_aabb(cs, ce, nb) : OBB ? q_box_near(cs.b, ce, nb)
                             : KIND == QK_DISC_CAST ? q_cast_aabb(ds, nb) : (DISC || KIND == QK_NEAR) ? q_disc_near(ds.c, nb) : q_overlap(nb, qbox);
                    }
                    if constexpr (KIND == QK_NEAR) {
                        float la = 0.f;
                        if (pass) {
                            la = q_near_gap(t.nodes[t.off[level - 1] + c], ds.c.cx, ds.c.cy);
                            pass = !(best_key != ~0ull && la > 0.f && la > q_funkey((unsigned)(best_key >> 32)));
                        }
                        const unsigned long long mask = __ballot(pass);
                        int below = 0;                                      // the passing children that are farther: they go under this one
                        for (unsigned long long rest = mask; rest; rest &= rest - 1) {
                            const int j = __builtin_ctzll(rest);
                            const float other = __shfl(la, j);
                            below += (other > la || (other == la && j < lane)) ? 1 : 0;
                        }
                        if (pass) st[sp + below] = ((unsigned)(level - 1) << 26) | (unsigned)c;
                        sp += __popcll(mask);
                        __builtin_amdgcn_wave_barrier();
                        continue;
                    }
                    const unsigned long long mask = __ballot(pass);
                    if (pass) st[sp + __popcll(mask & q_lanes_below())] = ((unsigned)(level - 1) << 26) | (unsigned)c;
                    sp += __popcll(mask);
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (KIND == QK_POINT) { best = q_wave_min(best); if (lane == 0) out_u32[q] = best; }
        if (KEY) { best_key = q_wave_min64(best_key); if (lane == 0) out_key[q] = best_key; }
        if (COUNT) { n_hits = q_wave_sum(n_hits); if (lane == 0) out_u32[q] = n_hits; }
        __builtin_amdgcn_wave_barrier();                                    // (the stack is reused by the wave's next query)
    }
}

// ascending order of each AABB segment of 2 .. Q_SORT_MAX hits: a workgroup per query (grid-strided), a bitonic sort in LDS
static __global__ void __launch_bounds__(256) k_qsort_segments(const unsigned* __restrict__ seg, const unsigned* __restrict__ len_of, int count, int* __restrict__ hits)
{
    __shared__ int s[Q_SORT_MAX];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {             // (q and len are uniform over the workgroup: the barriers below)
        const unsigned len = len_of[q];
        if (len <= 1u || len > (unsigned)Q_SORT_MAX) continue;
        int p = 1;
        while (p < (int)len) p <<= 1;
        int* h = hits + seg[q];
        for (int i = threadIdx.x; i < p; i += blockDim.x) s[i] = i < (int)len ? h[i] : INT_MAX;
        __syncthreads();
        for (int k = 2; k <= p; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < p; i += blockDim.x) {
                    const int l = i ^ j;
                    if (l > i) {
                        const int x = s[i], y = s[l];
                        if (((i & k) == 0) ? x > y : x < y) { s[i] = y; s[l] = x; }
                    }
                }
                __syncthreads();
            }
        for (int i = threadIdx.x; i < (int)len; i += blockDim.x) h[i] = s[i];
        __syncthreads();                                                    // (s is refilled for the next segment)
    }
}

} // namespace phx
